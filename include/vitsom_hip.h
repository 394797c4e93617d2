/* libvitsom_hip.so -- C-ABI of the MI355X-native ViT-SOM training-step kernels (gfx950 only).
 *
 * The reference (aluo7/ViT-SOM) is pure Python and has NO FFI/plugin interface;
 * each entry point below replaces the torch/ATen op sequence at the cited reference lines
 * (paths relative to the reference repo root).  A maintainer binds them with ctypes
 * (see INTEGRATION.md); the build's own host mirror lives in vit_som_amd/.
 *
 * Conventions (every entry):
 *   - returns 0 (VSOM_OK) on success, a negative VSOM_E* for a rejected call (bad shape,
 *     alignment, unsupported configuration, short workspace) or a positive hipError_t;
 *     vsom_last_error_string() describes the last failure on the calling thread;
 *   - all pointers are DEVICE pointers owned by the caller, fp32 row-major unless stated;
 *     BMU indices and labels are int64; "ld*" are row strides in ELEMENTS;
 *   - no allocation, no host synchronisation, no exceptions; work is enqueued on `stream`;
 *   - scratch is caller-supplied, sized by the matching *_workspace_bytes() query.
 */
#ifndef VITSOM_HIP_H
#define VITSOM_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ihipStream_t* vsom_stream_t; /* == hipStream_t */

#define VSOM_OK 0
#define VSOM_EINVAL (-1)       /* null pointer / non-positive or inconsistent shape */
#define VSOM_EALIGN (-2)       /* pointer or leading dimension not 16-byte aligned where required */
#define VSOM_EUNSUPPORTED (-3) /* configuration outside what the kernels implement */
#define VSOM_EWORKSPACE (-4)   /* workspace pointer null or too small */

#define VSOM_VERSION 100

#define VSOM_DIST_COSINE 0
#define VSOM_DIST_EUCLIDEAN 1
#define VSOM_DIST_MANHATTAN 2   /* torch.cdist(p=1) (models/som_layer.py:115-116; the DESOM configs' distance) */

int vsom_version(void);
const char* vsom_last_error_string(void);

/* ------------------------------------------------------------------ Linear layers
 * (fp32-accurate on the matrix cores: split-bf16 engine by default, exact-f32 MFMA on request -- vsom_set_gemm_mode) */
/* Y[M,N] = X[M,K] * W[N,K]^T + bias      -- nn.Linear forward: qkv models/vit.py:30,
 * decoder_pred vit.py:234, cls_head models/vit_som.py:77.  bias may be NULL.
 * Far pitches.  Every `ld` of this header is 64-bit: outputs, residuals and every operand of a kernel without a 16-byte
 * path are addressed with plain pointers at any pitch.  The two multiplied operands of a GEMM -- here and in
 * vsom_linear_gelu_fwd, vsom_linear_relu_fwd, vsom_linear_residual_fwd, vsom_linear_bwd_input, vsom_linear_bwd_input_t,
 * vsom_linear_bwd_weight, vsom_patch_embed_fwd, vsom_som_bwd, vsom_bmu_cosine_dots, vsom_bmu_cosine_fwd and
 * vsom_bmu_euclid_fwd -- are buffer resources with 32-bit byte offsets on the 16-byte path: operands of 4 GB or more take
 * the element-wise loads (from 0xFFFF0000 bytes, counted from the base to the end of the last row), without an error. */
int vsom_linear_fwd(const float* X, long ldx, const float* W, const float* bias, float* Y, long ldy,
                    int M, int N, int K, vsom_stream_t stream);

/* pre = X*W^T + bias ; Yact = gelu_erf(pre) ; Ygrad = gelu_erf'(pre)   -- mlp.0 + nn.GELU(),
 * vit.py:53-54.  The derivative is saved instead of the pre-activation (it is all the backward
 * needs, and both come from one exponential).  Both outputs dense [M,N]. */
int vsom_linear_gelu_fwd(const float* X, long ldx, const float* W, const float* bias, float* Ygrad,
                         float* Yact, int M, int N, int K, vsom_stream_t stream);

/* pre = X*W^T + bias ; Yact = max(pre, 0) ; Ygrad = (pre > 0) as 1.0 / 0.0   -- nn.Linear + nn.ReLU of the
 * DESOM autoencoder (models/ae.py:44-59).  Same contract as vsom_linear_gelu_fwd: the backward is
 * vsom_linear_bwd_input*(…, gelu_grad = Ygrad). */
int vsom_linear_relu_fwd(const float* X, long ldx, const float* W, const float* bias, float* Ygrad,
                         float* Yact, int M, int N, int K, vsom_stream_t stream);

/* Y[m] = X[m]*W^T + bias + R[m % r_mod]   -- Linear + residual add (attn.proj vit.py:38,61;
 * mlp.2 vit.py:55,62: r_mod = M, R = block input) and Linear + broadcast table
 * (decoder_embed + decoder_pos_embed vit.py:225-226: r_mod = tokens per image). */
int vsom_linear_residual_fwd(const float* X, long ldx, const float* W, const float* bias,
                             const float* R, long ldr, int r_mod, float* Y, long ldy, int M, int N,
                             int K, vsom_stream_t stream);

/* dX[M,K] (+)= dY[M,N] * W[N,K]  (optionally  .* gelu_grad[M,K], the Ygrad of vsom_linear_gelu_fwd)
 * -- autograd of nn.Linear w.r.t. its input (and of nn.GELU when gelu_grad != NULL, dense [M,K]). */
int vsom_linear_bwd_input(const float* dY, long lddy, const float* W, float* dX, long lddx, int M,
                          int N, int K, int accumulate, const float* gelu_grad, vsom_stream_t stream);

/* Same product from a TRANSPOSED weight copy Wt[K,N] (row-major, ld = N): both operands are then
 * contiguous along the reduction and the GEMM runs on the same kernel family as the forward
 * Linear (vsom_transpose_many keeps the copies current). */
int vsom_linear_bwd_input_t(const float* dY, long lddy, const float* Wt, float* dX, long lddx, int M,
                            int N, int K, int accumulate, const float* gelu_grad, vsom_stream_t stream);

/* Batched 2-D transpose: for i < count, dst_base[dst_off_i + c*rows_i + r] = src_base[src_off_i + r*cols_i + c].
 * `table` is a DEVICE array of count x 4 int64 {src_off, dst_off, rows, cols} (offsets in floats);
 * max_rows / max_cols bound every entry (they size the grid). */
int vsom_transpose_many(const float* src_base, float* dst_base, const long long* table, int count,
                        int max_rows, int max_cols, vsom_stream_t stream);

/* Arithmetic of the nn.Linear-shaped GEMMs (vsom_linear_*_fwd, vsom_linear_bwd_input_t, vsom_linear_bwd_weight,
 * vsom_patch_embed_*).  fp32 operands, fp32 accumulation and fp32 results in every mode:
 *   VSOM_GEMM_F32              v_mfma_f32_32x32x2_f32, bitwise an fmaf chain;
 *   VSOM_GEMM_SPLIT_BF16       every operand split EXACTLY into three bf16 pieces, the six leading cross products on
 *                              v_mfma_f32_32x32x16_bf16 (csrc/gemm_x6.h): dropped terms < 2^-22 relative -- fp32-accurate,
 *                              2.7x fewer matrix-core cycles than the f32 MFMA;
 *   VSOM_GEMM_SPLIT_BF16_GRAD3 (default) forward GEMMs exactly as VSOM_GEMM_SPLIT_BF16 -- outputs, logits, distances and
 *                              BMU indices are bit-identical to that mode -- while the Linear layers' weight-gradient and
 *                              input-gradient GEMMs (vsom_linear_bwd_weight, vsom_linear_bwd_input_t) use the two-piece
 *                              round-to-nearest split, three products: |error| <= 3 * 2^-16 per product in the worst case,
 *                              4e-6 relative on a weight gradient, 1e-5 on the gradients of the whole 12 + 2-layer step
 *                              (tools/accuracy_modes.py; the bar is 1e-4), half the matrix-core work of the backward GEMMs.
 * The cosine BMU pass has its own engines: vsom_bmu_cosine_x3_* (default: two-piece split, three products, exact
 * re-rank) and vsom_bmu_cosine_* (exact-f32 MFMA; what the host mirror uses in VSOM_GEMM_F32 mode and for the
 * euclidean distance).  Process-wide; returns VSOM_EINVAL on an unknown mode. */
#define VSOM_GEMM_F32 0
#define VSOM_GEMM_SPLIT_BF16 1
#define VSOM_GEMM_SPLIT_BF16_GRAD3 2
int vsom_set_gemm_mode(int mode);
int vsom_get_gemm_mode(void);
/* test / measurement hook for the weight-gradient GEMMs of VSOM_GEMM_SPLIT_BF16_GRAD3 mode whose output sides both
   divide by 192: 0 = the 192 x 64 tiles, 1 = 192 x 192 tiles at the split count of the 192 x 64 plan (bitwise the same
   dW and db; the GPU suite checks), 2 = 192 x 192 tiles with their own split count (default).  The workspace query
   follows the setting. */
int vsom_set_wgrad_tiles(int mode);
/* test / measurement hook for vsom_linear_bwd_input_ln{,_partial} at K = 192 in VSOM_GEMM_SPLIT_BF16_GRAD3 mode:
   0 = 64 x 192 tiles, 1 = 192 x 192 tiles (default).  dX and the partials are bitwise the same (the GPU suite checks);
   the partial layout and its size query do not depend on the setting.  Other values: VSOM_EINVAL. */
int vsom_set_ln_tiles(int mode);

/* Which kernel an entry point would launch ("Which kernel runs"), as one line of text in `out`:
 *     engine=<name> tile=<rows>x<cols> planes=<n> fast=<0|1> threads=<n> splits=<n> workgroups=<n>
 * engine: f32 | x6 (the generic GEMM kernels), x6_tn (weight-gradient tiles), x6_ln (LayerNorm-fused tiles), attn_two_launch
 * | attn_fused | attn_shared | attn_shared_bf16x3, bmu_x3 | bmu_x3_planes (the three-product BMU forms); planes = bf16 pieces per operand (0: fp32 products); fast = 16-byte
 * buffer loads.  Pure host arithmetic under the current GEMM mode and hooks: nothing is launched and no GPU is needed; the
 * library itself never calls it.  M, N, K are the entry point's own shape arguments in its own order ((B, K, L) for the SOM
 * entries; (N tokens, H, hd) for VSOM_PLAN_ATTENTION_BWD, workgroups per image).  flags bit 0: every operand is 16-byte
 * aligned with leading dimensions that are multiples of 4 (what the model's buffers are).  VSOM_EUNSUPPORTED where the
 * entry point would refuse the shape, VSOM_EINVAL on an unknown op, a non-positive shape or a buffer too small for the line. */
#define VSOM_PLAN_LINEAR_FWD 0
#define VSOM_PLAN_LINEAR_GELU_FWD 1
#define VSOM_PLAN_LINEAR_RELU_FWD 2
#define VSOM_PLAN_LINEAR_RESIDUAL_FWD 3
#define VSOM_PLAN_LINEAR_BWD_INPUT 4
#define VSOM_PLAN_LINEAR_BWD_INPUT_GELU 5
#define VSOM_PLAN_LINEAR_BWD_INPUT_T 6
#define VSOM_PLAN_LINEAR_BWD_INPUT_T_GELU 7
#define VSOM_PLAN_LINEAR_BWD_WEIGHT 8
#define VSOM_PLAN_LINEAR_BWD_INPUT_LN 9
#define VSOM_PLAN_SOM_BWD_GW 10
#define VSOM_PLAN_SOM_BWD_GX 11
#define VSOM_PLAN_BMU_COSINE_DOTS 12
#define VSOM_PLAN_ATTENTION_BWD 13
/* the cosine BMU pass as a whole, shape (B, K, L): engine = bmu_x3_planes | bmu_x3 | f32, the form vsom_bmu_cosine_form names
   for dense rows (ldx = L); flags bit 1: plane images are available.  VSOM_PLAN_BMU_COSINE_DOTS describes the exact entry
   point vsom_bmu_cosine_dots whatever the mode. */
#define VSOM_PLAN_BMU_COSINE 14
int vsom_describe_plan(int op, int M, int N, int K, int flags, char* out, size_t out_bytes);

/* dW[N,K] = dY[M,N]^T * X[M,K] ;  db[N] = column sums of dY (db may be NULL)
 * -- autograd of nn.Linear w.r.t. weight/bias.  The reduction over the M token rows is split
 * across workgroups into fp32 slabs in `ws` and summed in a fixed order (deterministic). */
size_t vsom_linear_bwd_weight_workspace_bytes(int M, int N, int K);
int vsom_linear_bwd_weight(const float* dY, long lddy, const float* X, long ldx, float* dW, float* db,
                           int M, int N, int K, void* ws, size_t ws_bytes, vsom_stream_t stream);

/* ------------------------------------------------------------------ patch embedding */
/* tokens[B, n+1, E]: row 0 = cls_token + pos[0]; row 1+i = Conv2d(k=s=p)(img)[patch i] + bias + pos[1+i]
 * -- timm PatchEmbed + vit.py:207-212.  img [B,C,S,S]; Wpe [E, C*p*p] (= conv weight [E,C,p,p]);
 * pos [n+1, E]; xp_ws [B*n, C*p*p] scratch that the backward re-uses (gathered patches). */
int vsom_patch_embed_fwd(const float* img, const float* Wpe, const float* bpe, const float* pos,
                         const float* cls_token, float* tokens, float* xp_ws, int B, int C, int S,
                         int p, int E, vsom_stream_t stream);
size_t vsom_patch_embed_bwd_workspace_bytes(int B, int C, int S, int p, int E);
/* dWpe, dbpe, dcls_token[E] from dtokens[B, n+1, E] (autograd of the above; pos is frozen). */
int vsom_patch_embed_bwd(const float* dtokens, const float* xp_ws, float* dWpe, float* dbpe,
                         float* dcls_token, int B, int C, int S, int p, int E, void* ws,
                         size_t ws_bytes, vsom_stream_t stream);

/* ------------------------------------------------------------------ LayerNorm */
/* Y = (X - mean)/sqrt(var + eps) * gamma + beta, rows x cols; saves mean/rstd per row.
 * -- nn.LayerNorm(eps=1e-6): vit.py:48,50,85,95 (eps from vit_som.py:50). cols <= 1024. */
int vsom_layernorm_fwd(const float* X, const float* gamma, const float* beta, float* Y, float* mean,
                       float* rstd, int rows, int cols, float eps, vsom_stream_t stream);
size_t vsom_layernorm_bwd_workspace_bytes(int rows, int cols);
/* dX = (resid ? resid : 0) + LN'(dY);  dgamma, dbeta = column reductions (deterministic). */
int vsom_layernorm_bwd(const float* dY, const float* X, const float* mean, const float* rstd,
                       const float* gamma, const float* resid, float* dX, float* dgamma, float* dbeta,
                       int rows, int cols, void* ws, size_t ws_bytes, vsom_stream_t stream);
/* The same in two halves (autograd of nn.LayerNorm, vit.py:48,50,85,95): _partial computes dX and leaves the column
 * partials in `part` (vsom_layernorm_bwd_workspace_bytes, kept by the caller); one vsom_layernorm_bwd_finish_many launch
 * then produces dgamma / dbeta for `count` such calls, bit for bit what vsom_layernorm_bwd would have written (the step's
 * 30 tiny reductions leave its critical chain).  jobs_dev: device array of VSOM_LN_JOB_WORDS 64-bit words per job --
 * part, dgamma, dbeta (pointers), (nblk << 32) | cols with nblk = workspace_bytes / (8 cols); jobs first .. first+count-1
 * are reduced, max_cols = the widest of them.  Shapes: vsom_layernorm_bwd_deferrable(rows, cols) != 0. */
#define VSOM_LN_JOB_WORDS 4
int vsom_layernorm_bwd_deferrable(int rows, int cols);
int vsom_layernorm_bwd_partial(const float* dY, const float* X, const float* mean, const float* rstd,
                               const float* gamma, const float* resid, float* dX, int rows, int cols, void* part,
                               size_t part_bytes, vsom_stream_t stream);
int vsom_layernorm_bwd_finish_many(const int64_t* jobs_dev, int first, int count, int max_cols, vsom_stream_t stream);

/* The input-gradient GEMM of vsom_linear_bwd_input_t (dY[M,N], Wt[K,N]) with the LayerNorm backward of its product in
 * the epilogue: dX = (resid ? resid : 0) + LN'(dY Wt^T) over rows of width K, in one launch -- the product never reaches
 * memory.  dX is bit for bit what vsom_linear_bwd_input_t into a scratch buffer followed by vsom_layernorm_bwd writes;
 * dgamma / dbeta come from per-row-tile partials (rounding differs from vsom_layernorm_bwd, the reduction is as
 * deterministic).  _partial leaves the partials in `part` for vsom_layernorm_bwd_finish_many (same job format, nblk =
 * part_bytes_query / (8 K)).  Supported (vsom_linear_bwd_input_ln_supported != 0): the split-bf16 GEMM modes, K = 192 or
 * 96, enough row tiles for the column reducer; otherwise VSOM_EUNSUPPORTED and the caller takes the two-launch path.
 * vsom_linear_bwd_input_ln and vsom_linear_bwd_input_ln_partial alike: dY, Wt, X, gamma, resid and dX 16-byte aligned,
 * lddy % 4 == 0 and N % 4 == 0 (VSOM_EALIGN otherwise: there is no element-wise form); X / resid / dX dense [M, K]; dY
 * (from its base to the end of its last row, at pitch lddy) and X below 4 GB (0xFFFF0000 bytes), VSOM_EUNSUPPORTED
 * otherwise, for the same reason. */
int vsom_linear_bwd_input_ln_supported(int M, int N, int K);
size_t vsom_linear_bwd_input_ln_partial_bytes(int M, int K);
int vsom_linear_bwd_input_ln(const float* dY, long lddy, const float* Wt, int M, int N, int K, const float* X,
                             const float* mean, const float* rstd, const float* gamma, const float* resid, float* dX,
                             float* dgamma, float* dbeta, void* ws, size_t ws_bytes, vsom_stream_t stream);
int vsom_linear_bwd_input_ln_partial(const float* dY, long lddy, const float* Wt, int M, int N, int K, const float* X,
                                     const float* mean, const float* rstd, const float* gamma, const float* resid,
                                     float* dX, void* part, size_t part_bytes, vsom_stream_t stream);

/* ------------------------------------------------------------------ multi-head attention */
/* out[B,N,H*hd] = softmax(q k^T * hd^-0.5) v, qkv laid out [B,N,3,H,hd] (the qkv Linear's
 * output, vit.py:30-37; dropout p=0).  lse[B,H,N] = log-sum-exp of the scaled scores (saved for
 * the backward, which recomputes the probabilities).  hd = 16, 32 or 64 (the 16-byte path): qkv and out 16-byte aligned,
 * else VSOM_EALIGN; hd <= 8 (element loads): any alignment. */
int vsom_attention_fwd(const float* qkv, float* out, float* lse, int B, int N, int H, int hd,
                       vsom_stream_t stream);
/* dqkv[B,N,3,H,hd] from dout[B,N,H*hd] (autograd of the above). delta_ws: [B,H,N] floats.  hd = 16, 32 or 64: qkv, out,
 * dout and dqkv 16-byte aligned, else VSOM_EALIGN; hd <= 8: any alignment. */
int vsom_attention_bwd(const float* qkv, const float* out, const float* dout, const float* lse,
                       float* dqkv, float* delta_ws, int B, int N, int H, int hd,
                       vsom_stream_t stream);
/* probs[B,H,N,N] = softmax(q k^T * hd^-0.5) -- the attention maps of `return_attn=True` (vit.py:33-34,41-42), formed
 * from qkv (the fused kernels never materialise them); each row is normalised by its own scores, `lse` must be a valid
 * pointer but is not read.  Visualisation path only. */
int vsom_attention_probs(const float* qkv, const float* lse, float* probs, int B, int N, int H, int hd,
                         vsom_stream_t stream);
/* test hook: 0 = run the short-sequence backward as two launches (dQ, then dK/dV), 1 = one launch whose phases share
   the scores (default), 2 = one launch that recomputes them: bit-identical results (the GPU suite checks) -- except that
   form 1, at hd = 64 in VSOM_GEMM_SPLIT_BF16_GRAD3 mode, forms its seven products on the bf16 matrix cores from the
   two-piece split of the gradient GEMMs (gradients within 8e-6 relative of fp64); 3 = form 1 with fp32 products always */
int vsom_set_attention_fused(int fused);

/* Single-query attention: ONE query row per (image, head) against the image's N keys -- the CLS row of a classifier's
 * last encoder block (classifier.py).  q[B,E] and kv[B*N,2E] (K then V) keep the qkv Linear's head interleave
 * (E = H*hd, head h in columns [h*hd, (h+1)*hd)); o[B,E] = softmax(q k^T * hd^-0.5) v, lse[B,H] = log-sum-exp of the
 * scaled scores.  hd in {8, 16, 32, 64}, any N >= 1; fp32 throughout; every output element written; no atomics
 * (bitwise reproducible).  q / kv / o 16-byte aligned. */
int vsom_attention_q1_fwd(const float* q, const float* kv, float* o, float* lse, int B, int N, int H, int hd,
                          vsom_stream_t stream);
/* dq[B,E] and dkv[B*N,2E] from dout[B,E] (autograd of the above); each (image, head) owns its rows of dkv.  dout / o / q /
 * kv / dkv 16-byte aligned (VSOM_EALIGN otherwise, as for q / kv / o above). */
int vsom_attention_q1_bwd(const float* dout, const float* o, const float* lse, const float* q, const float* kv, float* dq,
                          float* dkv, int B, int N, int H, int hd, vsom_stream_t stream);
/* dst[r, 0:cols] += src[r, 0:cols] for r < rows (row strides lds / ldd in floats): the CLS rows' residual gradient. */
int vsom_rows_add(const float* src, long lds, float* dst, long ldd, int rows, int cols, vsom_stream_t stream);

/* ------------------------------------------------------------------ SOM layer */
/* inv_norm[r] = 1 / max(||X[r,:]||_2, eps)   -- F.normalize(p=2, eps=1e-12), som_layer.py:120-121 */
int vsom_row_inv_norm(const float* X, long ldx, int rows, int cols, float eps, float* inv_norm,
                      vsom_stream_t stream);
/* sqnorm[r] = ||X[r,:]||_2^2  (for the euclidean distance) */
int vsom_row_sqnorm(const float* X, long ldx, int rows, int cols, float* sqnorm, vsom_stream_t stream);
/* Best-matching-unit search, cosine: dist[B,K] = 1 - (X/|X|)(W/|W|)^T ; bmu[b] = first argmin_k
 * -- SOMLayer.compute_distances + forward, som_layer.py:83-89,119-122.  X [B,L] (row stride ldx:
 * the patch tokens of image b are contiguous), W [K,L] dense.  dist may be NULL. */
size_t vsom_bmu_cosine_workspace_bytes(int B, int K, int L);
int vsom_bmu_cosine_fwd(const float* X, long ldx, const float* W, const float* inv_nx,
                        const float* inv_nw, float* dist, int64_t* bmu, int B, int K, int L, void* ws,
                        size_t ws_bytes, vsom_stream_t stream);
/* The two halves of vsom_bmu_cosine_fwd, callable separately (bench.py times the distance pass
 * alone): _dots = the [B,L]x[L,K] contraction, split over L into fp32 partial slabs in ws;
 * _finalize = slab sum, 1 - dot * inv_nx * inv_nw, first-argmin. */
int vsom_bmu_cosine_dots(const float* X, long ldx, const float* W, int B, int K, int L, void* ws,
                         size_t ws_bytes, vsom_stream_t stream);
int vsom_bmu_cosine_finalize(const void* ws, size_t ws_bytes, const float* inv_nx, const float* inv_nw,
                             float* dist, int64_t* bmu, int B, int K, int L, vsom_stream_t stream);
/* Best-matching-unit search, euclidean: dist = torch.cdist(X, W, p=2) in its matmul form
 * sqrt(|x|^2 + |w|^2 - 2 x.w) (torch.cdist's matmul form) -- som_layer.py:117-118; same workspace as cosine.  A squared
 * distance at or below 2^-20 (|x|^2 + |w|^2) -- the rounding noise of this form -- is reported as exactly 0, and the
 * SOM backward gives the subgradient 0 there (torch's at d == 0): a sample within ~1e-3 sqrt(|x|^2 + |w|^2) of a prototype
 * neither pulls nor is pulled by it, where torch's clamp_min(1e-30) would return noise or 1e-15.  NaN stays NaN. */
int vsom_bmu_euclid_fwd(const float* X, long ldx, const float* W, const float* sq_x, const float* sq_w,
                        float* dist, int64_t* bmu, int B, int K, int L, void* ws, size_t ws_bytes,
                        vsom_stream_t stream);
/* Neighbourhood weights + SOM loss + backward coefficients in one pass over [B,K]:
 *   h_ik = exp(-||g_k - g_bmu(i)||^2 / (2 T^2))              compute_weights, som_layer.py:144-152
 *   loss_sum[0] = sum_ik h_ik d_ik   (caller divides by B*K)  som_loss, som_layer.py:137-142
 *   (all loss sums are two-stage fixed-order reductions: bitwise reproducible)
 *   coef[i,k] = -c * h_ik * inv_nx[i] * inv_nw[k],  c = grad_scale
 *   row_dot[i] = c * inv_nx[i]^2 * sum_k h_ik (1 - d_ik);  col_dot[k] likewise over i
 * (distance = VSOM_DIST_EUCLIDEAN: coef = -c h/d, row_dot = c sum_k h/d, col_dot = c sum_i h/d, the
 *  coefficients of d|x-w|; inv_nx / inv_nw are then unused and vsom_som_bwd applies unchanged)
 * h may be NULL; coef/row_dot/col_dot may all be NULL (forward only).  grid [K,2] float. */
size_t vsom_som_neigh_workspace_bytes(int B, int K);
int vsom_som_neigh_loss(const float* dist, const int64_t* bmu, const float* grid, float T,
                        const float* inv_nx, const float* inv_nw, float grad_scale, float* h,
                        float* loss_sum, float* coef, float* row_dot, float* col_dot, int B, int K,
                        int distance, void* ws, size_t ws_bytes, vsom_stream_t stream);
/* Prototype gradient ("per-BMU neighbourhood accumulator") and input gradient of
 * gamma_t * mean(h * d) through both F.normalize calls:
 *   gW[K,L]  = coef^T X + col_dot[k] * W[k,:]
 *   gX[B,L] += coef  W + row_dot[i] * X[i,:]        (accumulated into the token gradient) */
int vsom_som_bwd(const float* X, long ldx, const float* W, const float* coef, const float* row_dot,
                 const float* col_dot, float* gW, float* gX, long ldgx, int accumulate_gx, int B, int K,
                 int L, vsom_stream_t stream);

/* manhattan BMU search: dist[B,K] = sum_l |X[i,l] - W[k,l]| (torch.cdist p=1, som_layer.py:115-116),
 * bmu = first argmin.  Tiled VALU kernels (|x - w| has no dot-product form); the reduction over l is
 * split into fp32 slabs in `ws`, summed in a fixed order.  dist may be NULL. */
size_t vsom_bmu_manhattan_workspace_bytes(int B, int K, int L);
int vsom_bmu_manhattan_fwd(const float* X, long ldx, const float* W, float* dist, int64_t* bmu, int B, int K,
                           int L, void* ws, size_t ws_bytes, vsom_stream_t stream);

/* Backward of som_loss through the manhattan distances, from coef = dLoss/d dist written by
 * vsom_som_neigh_loss(distance = VSOM_DIST_MANHATTAN):
 *   gW[k,l]   = -sum_i coef[i,k] sign(X[i,l] - W[k,l])
 *   gX[i,l] (+)= sum_k coef[i,k] sign(X[i,l] - W[k,l])          (sign(0) = 0, as torch) */
int vsom_som_bwd_manhattan(const float* X, long ldx, const float* W, const float* coef, float* gW, float* gX,
                           long ldgx, int accumulate_gx, int B, int K, int L, vsom_stream_t stream);

/* ------------------------------------------------------------------ losses */
/* loss_sum[0] = sum_i |pred[i] - target[i]| over n elements (nn.L1Loss numerator, models/desom.py:44,146);
 * dpred[i] = grad_scale * sign(pred[i] - target[i]) when dpred != NULL.  Fixed-order reduction through `ws`. */
size_t vsom_l1_loss_workspace_bytes(long n);
int vsom_l1_loss(const float* pred, const float* target, float* loss_sum, float* dpred, float grad_scale, long n,
                 void* ws, size_t ws_bytes, vsom_stream_t stream);

/* L1Loss(unpatchify(pred[:,1:,:]), img) -- vit.py:141-153,234-236 + vit_som.py:100.
 * pred [B, n+1, p*p*C] (row 0 of each image = CLS prediction, ignored); img [B,C,S,S].
 * recon [B,C,S,S] (may be NULL); loss_sum[0] = sum |recon-img| (caller divides by B*C*S*S);
 * dpred (may be NULL) = grad_scale * sign(recon-img) in pred layout, CLS rows zero. */
size_t vsom_l1_unpatchify_workspace_bytes(int B, int C, int S, int p);
int vsom_l1_unpatchify(const float* pred, const float* img, float* recon, float* loss_sum,
                       float* dpred, float grad_scale, int B, int C, int S, int p, void* ws,
                       size_t ws_bytes, vsom_stream_t stream);
/* CrossEntropyLoss(label_smoothing=s)(logits[B,C], y[B]) -- vit_som.py:62,96.
 * loss_sum[0] = sum_b loss_b (caller divides by B); dlogits (may be NULL) = grad_scale * dloss_b/dlogits. */
size_t vsom_cross_entropy_ls_workspace_bytes(int B);
int vsom_cross_entropy_ls(const float* logits, const int64_t* y, float smoothing, float* loss_sum,
                          float* dlogits, float grad_scale, int B, int C, void* ws, size_t ws_bytes,
                          vsom_stream_t stream);

/* ------------------------------------------------------------------ optimiser */
/* One decoupled-weight-decay Adam step over a flat fp32 arena (torch.optim.AdamW semantics,
 * vit_som.py:146-151).  wd_per_chunk[i] is the weight decay of elements [256 i, 256 i + 256);
 * adamw=0 selects torch.optim.Adam (L2 in the gradient).  g is multiplied by grad_scale first
 * (1/world_size after a sum all-reduce).  n a multiple of 256; p, g, m and v 16-byte aligned (VSOM_EALIGN otherwise:
 * the arena is walked 16 bytes at a time and has no element-wise form). */
int vsom_adamw_step(float* p, const float* g, float* m, float* v, const float* wd_per_chunk, long n,
                    float lr, float beta1, float beta2, float eps, int step, float grad_scale,
                    int adamw, vsom_stream_t stream);

/* ------------------------------------------------------------------ data-parallel exchange (RCCL over xGMI) */
/* One process per GPU, one communicator per process.  Replaces the implicit DDP gradient all-reduce of the reference
 * (experiments/benchmarking/train_vit_som.py:44-45,86-91: DEVICES > 1 -> Lightning DDPStrategy -> NCCL).  RCCL is bound
 * at run time (dlopen; a copy already in the process, e.g. torch.distributed's, is shared; VSOM_RCCL_PATH overrides).
 *   vsom_comm_unique_id   rank 0 fills `id_out` (HOST memory, VSOM_COMM_ID_BYTES); the host distributes it to all ranks
 *   vsom_comm_init        collective: every rank calls it with the same id (the current HIP device is the rank's GPU)
 *   vsom_comm_allreduce_sum  in-place sum of buf[0..n) over the ranks, enqueued on `stream` (no host sync): the host
 *                         mirror calls it per arena slice as the backward finishes it (ViT gradients and the [K,L]
 *                         prototype accumulators alike); AdamW then applies grad_scale = 1/world_size
 *   vsom_comm_info        world_size / rank of the live communicator (0 / -1 when none)
 *   vsom_comm_destroy     releases it (idempotent) */
#define VSOM_COMM_ID_BYTES 128
int vsom_comm_unique_id(void* id_out);
int vsom_comm_init(const void* unique_id, int world_size, int rank);
int vsom_comm_allreduce_sum(float* buf, long n, vsom_stream_t stream);
int vsom_comm_info(int* world_size, int* rank);
int vsom_comm_destroy(void);

/* ------------------------------------------------------------------ launch tape (the step as ONE host call per segment) */
/* The reference drives its step from Python through ATen, one host round trip per op (vit_som.py:80-105 under Lightning's fit
 * loop); so does the host mirror, ~420 launches and ~4 ms of host time per step -- more than the GPU needs below ~256 images
 * per GPU (BASELINE c4 at 128 per GPU, c3 read as 512 global).  A tape records the launches of one step WHILE THEY RUN and
 * re-issues them from C:
 *   vsom_tape_begin      start recording on the calling thread; returns the tape id (> 0).  Every launch any vsom_* entry
 *                        makes on this thread from now on is executed AND kept (kernel, grid, LDS, stream, by-value arguments),
 *                        as are vsom_event_record / vsom_stream_wait_event and vsom_comm_allreduce_sum
 *   vsom_tape_cut        close the current segment, open the next; returns the index of the closed one
 *   vsom_tape_pause      1: execute but do not keep what follows (calls whose arguments change per step), 0: resume
 *   vsom_tape_end        stop recording; returns the number of segments
 *   vsom_tape_replay     re-issue one segment's operations in order (per launch: hipLaunchKernel + hipGetLastError).  Each
 *                        operation's status is checked (launch, event record / wait, RCCL; an all-reduce with no live
 *                        communicator is refused before RCCL is called): the replay stops at the first failure and returns
 *                        its status, the error string naming the segment, the operation's index and what it is
 *   vsom_tape_segment_ops / vsom_tape_recording (0 no, 1 recording, 2 paused) / vsom_tape_destroy
 * Pointers are frozen into the tape: the caller replays only while every buffer the recorded step touched is alive and in
 * place (the host mirror stages each batch into fixed input buffers and ties the tape to its activation buffers).
 *   vsom_event_record / vsom_stream_wait_event: library-owned events (ids 0..511, created on first use) for the edges
 *   between the step's HIP streams, so that they are part of a tape. */
int vsom_tape_begin(void);
int vsom_tape_cut(void);
int vsom_tape_pause(int paused);
int vsom_tape_end(void);
int vsom_tape_recording(void);
int vsom_tape_segment_ops(int tape, int segment);
int vsom_tape_replay(int tape, int segment);
int vsom_tape_destroy(int tape);
int vsom_event_record(int ev, vsom_stream_t stream);
int vsom_stream_wait_event(vsom_stream_t stream, int ev);

/* ------------------------------------------------------------------ evaluation (tools/evaluation.py) */
/* table[a[i] * nb + b[i]] += 1 for i < n  (uint64 counts, accumulates: zero it before the first
 * batch) -- the contingency matrix of calculate_purity (evaluation.py:142-145) and of the
 * classification metrics.  Entries outside [0,na) x [0,nb) are counted in out_of_range[0]. */
int vsom_contingency(const int64_t* a, const int64_t* b, long n, int na, int nb,
                     unsigned long long* table, int* out_of_range, vsom_stream_t stream);
/* out[r] = first argmax_c X[r,c] -- torch.argmax(cls_logits, dim=1), evaluation.py:119 */
int vsom_argmax_rows(const float* X, long ldx, int rows, int cols, int64_t* out, vsom_stream_t stream);

/* Decoder output -> pictures, for visualize_decoded_prototypes (evaluation.py:153-222).  pred is what decoder_pred
 * wrote for `chunk` images: [chunk * (n + 1), p*p*C] contiguous, a CLS row in front of each image's n = g*g patch rows.
 * Image i of the chunk is prototype k0 + i of K.  The CLS row is dropped and unpatchify's index map (vit.py:141-153,
 * nhwpqc -> nchpwq) applied; S = g * p.  Either or both outputs (the other NULL):
 *   images  f32 [K, C, S, S]: images[k0 + i] = the unpatchified values, bit for bit;
 *   canvas  uint8 RGB [rows*S + (rows-1)*gap, cols*S + (cols-1)*gap, 3], rows * cols == K: prototype k at cell
 *           divmod(k, cols) (axes.flatten() order), level floor(255 t + 0.5) with t as imshow forms it:
 *           C == 3: clip(v, 0, 1) per channel; C == 1: (v - min) / (max - min) over that image, on all three channels,
 *           0 for a constant image.  Each image also writes the 255 strip to its right and below it (none at the
 *           last column / row), so K images fill the whole canvas.
 * Other channel counts: VSOM_EUNSUPPORTED. */
int vsom_proto_mosaic(const float* pred, int chunk, int n, int p, int C, float* images, unsigned char* canvas, int k0,
                      int K, int rows, int cols, int gap, vsom_stream_t stream);
/* The label of the LAST sample that lands on each map cell (evaluation.py:254-258 `heatmap[divmod(bmu)] = label` in
 * sample order), order-independent: cells[bmu[i]] = max(cells[bmu[i]], (first_ordinal + i + 1) << 32 | label[i]) for
 * i < n (integer atomic max; zero `cells` [K] before the first batch; a cell never hit stays 0 and decodes to label 0).
 * first_ordinal = the number of samples in the batches before this one; ordinals stay below 2^31, so the words are
 * positive as int64 too and tables of several ranks combine with one MAX all-reduce.  A bmu outside [0, K) or a
 * label outside [0, 2^31) is counted in out_of_range[0] and not written. */
int vsom_last_label(const int64_t* bmu, const int64_t* label, long n, long first_ordinal, int K,
                    unsigned long long* cells, int* out_of_range, vsom_stream_t stream);

/* Map quality (no counterpart in the reference): one fold per batch over what the BMU pass left, no host synchronisation.
 * dist [B, K] f32 (row stride K), bmu [B] int64, grid_positions [K, 2] f32 (the layer's buffer).  The accumulators are
 * zeroed by the caller once per evaluation (nearest: all-ones = "no sample"); the kernel only adds, or min-folds nearest:
 *   second[i]  (optional, NULL to skip) = first argmin over k != bmu[i] of dist[i, k] (float comparison: -0.0 == 0.0;
 *              lowest index on a tie) -- exact on the dist it is given;
 *   te[0]     += 1 when |pos[bmu[i]] - pos[second[i]]|^2 > adj_r2 (fp64 arithmetic on the fp32 positions);
 *   hits[b]   += 1, qe_fix[b] += llrint(dist[i, b] * 2^32) for b = bmu[i]: fixed point, so the sums do not depend on the
 *              order the atomics land in (per cell, sum |dist| must stay below 2^31);
 *   nearest[k] = min over ALL samples i of (ordered_key(dist[i, k]) << 32) | (first_ordinal + i), ordered_key(v) =
 *              bits(v) with the sign bit set for v >= +0, ~bits(v) otherwise: order-preserving on fp32 (-0.0 below
 *              +0.0); ties go to the lowest ordinal.
 * A row with bmu outside [0, K), a NaN distance or |dist[i, bmu]| >= 2^31 is counted in bad[0] and skipped entirely.
 * K < 2: VSOM_EINVAL.  first_ordinal + B >= 2^31: VSOM_EUNSUPPORTED.  B == 0: nothing is launched.
 * Rows are read 16 bytes per lane when K % 4 == 0 and dist is 16-byte aligned. */
int vsom_map_stats(const float* dist, const int64_t* bmu, long B, int K, const float* grid_positions, float adj_r2,
                   long first_ordinal, long long* hits, long long* qe_fix, long long* te, unsigned long long* nearest,
                   int* bad, int64_t* second, vsom_stream_t stream);
/* U-matrix: for every unit k of W [K, L] (f32, contiguous) the units j != k with |pos_j - pos_k|^2 <= adj_r2 in ascending
 * index order -> nbr_idx [K, 8] int32 (padded with -1), their distance to unit k -> nbr_dist [K, 8] f32 (0 in the padding)
 * and u [K] f32 = the mean of the valid entries, summed in slot order in fp64 (0 for a unit with no neighbour).
 * Distances are accumulated over the whole row in fp64 from exact products / differences of the fp32 values, in a fixed
 * order, and rounded to fp32 once:  VSOM_DIST_COSINE 1 - <a,b> / (max(|a|, 1e-12) max(|b|, 1e-12));  VSOM_DIST_EUCLIDEAN
 * sqrt(sum (a - b)^2) (the difference form: neighbouring prototypes are close);  VSOM_DIST_MANHATTAN sum |a - b|.
 * Any other distance: VSOM_EUNSUPPORTED.  A unit with more than 8 units within adj_r2 cannot be known on the host (the
 * positions live on the device): the kernel keeps the first 8 and raises status[0] (zeroed by the caller) to the largest
 * count seen; the caller reads it after the launch and treats a non-zero value as VSOM_EUNSUPPORTED.
 * Rows are read 16 bytes per lane when L % 4 == 0 and W is 16-byte aligned. */
int vsom_umatrix(const float* W, int K, int L, const float* grid_positions, float adj_r2, int distance, int* nbr_idx,
                 float* nbr_dist, float* u, int* status, vsom_stream_t stream);

/* k-means of evaluate_kmeans (evaluation.py:54-91): the data-touching steps of sklearn.cluster.KMeans
 * (sklearn/cluster/_kmeans.py, algorithm="lloyd", dense fp32, unit sample weights).  X is [N, D] with row stride ldx;
 * centres are [k, D] contiguous; labels int64.  Every sum has a fixed order (no floating-point atomics): results are
 * bitwise reproducible.  One workspace of vsom_kmeans_workspace_bytes(N, D, k) bytes serves every entry below
 * (host arithmetic only; 0 for a non-positive size). */
size_t vsom_kmeans_workspace_bytes(long N, int D, int k);
/* One Lloyd E-step and the partial M-step in one launch (_k_means_lloyd.pyx lloyd_iter_chunked_dense; each row is read
 * twice, the second time for the M-step shortly after the first):
 * labels[i] = first argmin_j |x_i - c_j|^2 (fp32 sum of squared differences; ties -> lowest j), mind[i] = that
 * distance, and into the workspace: per-workgroup cluster sums / counts and the number of i with
 * labels[i] != prev_labels[i] (prev_labels may alias labels).  k <= 1024. */
int vsom_kmeans_assign(const float* X, long ldx, long N, int D, const float* centers, int k, int64_t* labels,
                       const int64_t* prev_labels, float* mind, void* ws, size_t ws_bytes, vsom_stream_t stream);
/* After vsom_kmeans_assign with the same (N, D, k, ws): the per-workgroup partials reduced in fixed order into
 * counts[k] and centers_new = sums * (1 / counts) (_average_centers: an empty cluster takes the row of the first
 * argmax of counts, averaged if that cluster comes before it and its raw sum if after, as sklearn's in-place loop), and
 * status[4] (fp64) = {labels changed, center_shift_tot = sum |new - old|^2 (_kmeans_single_lloyd),
 * empty clusters, inertia = sum_i mind[i] (_inertia)}. */
int vsom_kmeans_update(const float* centers_old, float* centers_new, long N, int D, int k, const float* mind,
                       int64_t* counts, double* status, void* ws, size_t ws_bytes, vsom_stream_t stream);
/* _relocate_empty_clusters_dense after vsom_kmeans_update found empty clusters: moves[2m] = an empty cluster,
 * moves[2m+1] = the far sample the host chose for it (argpartition of mind), applied in order to the reduced sums
 * and counts; then centers_new, status[1] (shift) and status[2] (clusters still empty) again. */
int vsom_kmeans_relocate(const float* X, long ldx, long N, int D, int k, const int64_t* labels, const int64_t* moves,
                         int n_moves, const float* centers_old, float* centers_new, int64_t* counts, double* status,
                         void* ws, size_t ws_bytes, vsom_stream_t stream);
/* _kmeans_plusplus' candidate step: dist[t][i] = min(closest[i], |x_i - x_{candidates[t]}|^2) (closest may be NULL:
 * no minimum) and pots[t] = sum_i dist[t][i] (fp64, fixed order), for t < n_candidates <= 64. */
int vsom_kmeanspp_dist(const float* X, long ldx, long N, int D, const int64_t* candidates, int n_candidates,
                       const float* closest, float* dist, double* pots, vsom_stream_t stream);
/* _tolerance: out[0] = mean over columns of var(X, axis=0) (fp64); workspace as for (N, D, k). */
int vsom_kmeans_colvar(const float* X, long ldx, long N, int D, int k, double* out, void* ws, size_t ws_bytes,
                       vsom_stream_t stream);

/* UMAP of visualize_umap_progression (evaluation.py:267-323; vit_som_amd/umap.py states the algorithm).  No
 * floating-point atomics, every sum in one fixed order: a fit is bitwise reproducible.
 * Exact k nearest neighbours of every row of X [N, D] (row stride ldx) among all rows: knn_idx int64 [N, k] and
 * knn_dist f32 [N, k] ascending by (distance, index), row i itself first with distance 0 (its duplicates follow).
 * metric VSOM_DIST_EUCLIDEAN: the true distance sqrt(max(|x|^2 + |y|^2 - 2 <x,y>, 0)); VSOM_DIST_COSINE:
 * 1 - <x,y> / (|x| |y|) clamped at 0, 0 when both rows are zero and 1 when exactly one is.  <x,y> is an f32 matrix-core
 * contraction; the squared norms are summed in its order, so identical rows are at distance exactly 0.
 * This is the search of vsom_knn_query with the set as its own bank (one kernel, csrc/knn.hip); only here is row i put
 * first.  Rows are loaded under the conditions of vsom_knn_query: operands of 4 GB or more take the element-wise loads.
 * 1 <= k <= 64, k < N.  Workspace: vsom_umap_knn_workspace_bytes(N, k) (host arithmetic; 0 for a non-positive size): the
 * N squared norms and two candidate slabs (f32 distances, i32 rows) of chunks * rb * 128 * k entries each, rb =
 * ceil(N / 128) row blocks and chunks = min(ceil(N / 64), ceil(2048 / rb)) column chunks, every section rounded up to
 * 256 bytes; at least 8 N k bytes. */
size_t vsom_umap_knn_workspace_bytes(long N, int k);
int vsom_umap_knn(const float* X, long ldx, long N, int D, int k, int metric, int64_t* knn_idx, float* knn_dist, void* ws,
                  size_t ws_bytes, vsom_stream_t stream);
/* Negative sample p of edge `edge` in epoch `epoch` (host arithmetic, the function vsom_umap_epoch evaluates):
 *   splitmix64(z) = z += 0x9E3779B97F4A7C15; z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9; z = (z ^ z >> 27) * 0x94D049BB133111EB;
 *                   z ^ z >> 31                                                    (all mod 2^64)
 *   sample = splitmix64(splitmix64(seed ^ edge) ^ (epoch << 32 | p)) mod N         (epoch, p < 2^32)
 * -1 for a negative argument or N < 1. */
long vsom_umap_neg_sample(uint64_t seed, int epoch, long edge, long p, long N);
/* One layout epoch n = `epoch` of optimize_layout_euclidean (move_other) with synchronous updates.  The graph is a
 * symmetric CSR (indptr int64 [N+1], indices int64); per edge e = (v, u) fp64 epochs_per_sample, epoch_of_next_sample,
 * epochs_per_negative_sample, epoch_of_next_negative_sample (the two "next" arrays are updated in place).  Y_in / Y_out
 * [N, dim] f32 (must not alias).  For every vertex v, in CSR order over its edges with next_e <= n:
 *   attraction  d2 = |y_v - y_u|^2, c = -2ab d2^(b-1) / (a d2^b + 1) (0 if d2 == 0), term = clip(c (y_v - y_u), -4, 4)
 *               per component, added twice (the reverse edge's "move other" update of v is the same term);
 *   next_e += epochs_per_sample_e; n_neg = floor((n - next_neg_e) / epochs_per_negative_sample_e);
 *   repulsion   for p < n_neg: s = vsom_umap_neg_sample(seed, n, e, p, N), d2 = |y_v - y_s|^2,
 *               c = 2 gamma b / ((0.001 + d2)(a d2^b + 1)), term = clip(c (y_v - y_s), -4, 4); skipped when d2 == 0;
 *   next_neg_e += n_neg * epochs_per_negative_sample_e;
 * then Y_out[v] = y_v + alpha * (the terms summed in that order).  Every term reads Y_in.  1 <= dim <= 4. */
int vsom_umap_epoch(const int64_t* indptr, const int64_t* indices, const double* epochs_per_sample,
                    double* epoch_of_next_sample, const double* epochs_per_negative_sample,
                    double* epoch_of_next_negative_sample, const float* Y_in, float* Y_out, long N, int dim, float a,
                    float b, float gamma, float alpha, int epoch, uint64_t seed, vsom_stream_t stream);
/* The layout of UMAP.transform (optimize_layout_euclidean, move_other=False): M new points against the fixed training
 * embedding Y_train [N, dim] f32, epochs epoch_begin .. epoch_end - 1 of an n_epochs schedule in ONE launch, one thread
 * per new point (the points never interact).  knn_idx int64 [M, k] are ordinals of training rows, weights fp64 [M, k]
 * the row-normalised memberships, epochs_per_sample fp64 [M, k] (+inf = a pruned edge, never sampled); Y [M, dim] f32 is
 * read (epoch_begin > 0) and written.  The schedule state lives in ws: epoch_of_next_sample fp64 [k][M] at offset 0 and
 * epoch_of_next_negative_sample fp64 [k][M] at offset round_up(8 M k, 256), and persists there between calls.
 * epoch_begin == 0 first writes Y[i] = sum_j weights[i,j] Y_train[knn_idx[i,j]] (fp64, j = 0 .. k-1 in order, rounded once)
 * and resets the state to next = eps, next_neg = eps / negative_sample_rate.  Then for n = epoch_begin .. epoch_end - 1
 * and j = 0 .. k-1 in order, when next[j] <= n:
 *   attraction  to u = knn_idx[i,j]: d2 = |y - y_u|^2, c = -2ab d2^(b-1) / (a d2^b + 1) (0 if d2 == 0),
 *               y += alpha_n clip(c (y - y_u), -4, 4), applied at once and once;
 *   next[j] += eps[j]; n_neg = floor((n - next_neg[j]) / (eps[j] / negative_sample_rate));
 *   repulsion   for p < n_neg, each applied at once: s = vsom_umap_neg_sample(seed, n, i k + j, p, N), d2 = |y - y_s|^2,
 *               c = 2 gamma b / ((0.001 + d2)(a d2^b + 1)), y += alpha_n clip(c (y - y_s), -4, 4); nothing when d2 == 0;
 *   next_neg[j] += n_neg * (eps[j] / negative_sample_rate).
 * alpha_0 = initial_alpha, alpha_n = initial_alpha (1 - (n-1) / n_epochs), computed in fp64 and rounded to f32.  So
 * [0, e) followed by [e, n) on the same ws and Y is [0, n) bit for bit.  transform_graph (vit_som_amd/umap.py) gives
 * eps >= 1; a call's run time grows with n_epochs negative_sample_rate / eps.
 * An edge with an ordinal outside [0, N), a NaN or negative weight, or a NaN or non-positive eps is never followed (not
 * in the initial sum either; its state is +inf) and counted in status[0] (int32 [1], zeroed by the caller) once per call.
 * 1 <= k <= 64 (more: VSOM_EUNSUPPORTED), 1 <= dim <= 4, M, N >= 1, 0 <= epoch_begin <= epoch_end <= n_epochs,
 * negative_sample_rate >= 1.  Workspace: vsom_umap_transform_workspace_bytes(M, k) (host arithmetic; 0 for a non-positive
 * size); too small or NULL: VSOM_EWORKSPACE. */
size_t vsom_umap_transform_workspace_bytes(long M, int k);
int vsom_umap_transform_layout(const int64_t* knn_idx, const double* weights, const double* epochs_per_sample,
                               const float* Y_train, long N, float* Y, long M, int k, int dim, float a, float b, float gamma,
                               double initial_alpha, int n_epochs, int epoch_begin, int epoch_end, int negative_sample_rate,
                               uint64_t seed, int32_t* status, void* ws, size_t ws_bytes, vsom_stream_t stream);

/* k-nearest-neighbour probe of evaluate_knn (no counterpart in the reference).  No floating-point atomics, every sum in
 * one fixed order: two runs are bitwise equal.
 * For every row of Q [Nq, D] (row stride ldq) the k nearest rows of the bank chunk X [Nb, D] (row stride ldx):
 * idx int64 [Nq, k] = index_base + row, dist f32 [Nq, k], ascending by (distance, index).  Distances are those of
 * vsom_umap_knn (same metrics, same zero-row conventions, an f32 matrix-core contraction with the squared norms summed
 * in its order: a query identical to a bank row is at exactly 0); any other metric: VSOM_EUNSUPPORTED.  Unlike there
 * nothing is put first artificially.
 * accumulate == 0: the lists start empty, an empty slot being (+inf, -1).  accumulate != 0: idx / dist hold on entry a
 * result of earlier calls over OTHER index ranges and are folded with this chunk.  The dot product of a (query, bank
 * row) pair is summed in one order over D that depends neither on where the rows fall in a tile, nor on Nq, Nb or the
 * chunking, so a bank streamed in any number of pieces, in any order, gives bit for bit the lists of one call over the
 * whole bank.  Nb < k is legal: the unfilled tail stays (+inf, -1).
 * Bad rows (here, in vsom_umap_knn and in vsom_knn_ranks): a pair with a row that holds a NaN or an infinity, or whose
 * squared norm (euclidean: squared distance) overflows fp32, has no distance.  It is never listed and never counted: a
 * bad bank row is in no list, a bad query's list is all (+inf, -1) (vsom_umap_knn: row i at 0, then empty slots), and
 * every other query's list is bit for bit that of the call with the bad rows deleted; vsom_knn_ranks gives a slot that
 * names a bad row, and every slot of a bad row, less = tied = -1.  Every listed distance is finite and >= 0.
 * exclude (may be NULL): exclude[i] is a global bank ordinal that query i never receives (leave-one-out when queries
 * and bank are the same set).
 * 1 <= k <= 64 (more: VSOM_EUNSUPPORTED); 1 <= Nq, Nb <= 2^31 - 129; ldq, ldx >= D >= 1; index_base >= 0.  Rows are
 * loaded 16 bytes per lane when D % 4 == 0 and both pointers and strides are 16-byte aligned, element-wise otherwise;
 * operands of 4 GB or more take the element-wise loads too (rows * ld * 4 bytes from 0xFFFFFFF0 - 256, no error).
 * Workspace: vsom_knn_query_workspace_bytes(Nq, Nb, k) (host arithmetic, monotone in each argument; 0 for a
 * non-positive size); too small or NULL: VSOM_EWORKSPACE. */
size_t vsom_knn_query_workspace_bytes(long Nq, long Nb, int k);
int vsom_knn_query(const float* Q, long ldq, long Nq, const float* X, long ldx, long Nb, int D, int k, int metric,
                   int64_t index_base, int accumulate, const int64_t* exclude, int64_t* idx, float* dist, void* ws,
                   size_t ws_bytes, vsom_stream_t stream);
/* Neighbour ranks (trustworthiness / continuity of an embedding, vit_som_amd/embedding_quality.py; no counterpart in the
 * reference).  d(i, l) is the distance of vsom_umap_knn between rows i and l of A [N, D] (row stride lda), computed by
 * the same contraction in the same summation order.  nbr int64 [N, k] lists, for every row, k rows of the same set (the
 * neighbours it has in ANOTHER space); for every slot with n = nbr[i][j] in [0, N), n != i:
 *   less[i][j] = #{ l : l != i, l != n, d(i, l) <  d(i, n) }      (int32 [N, k])
 *   tied[i][j] = #{ l : l != i, l != n, d(i, l) == d(i, n) }      (int32 [N, k])
 * so that n has rank 1 + less (ties to the lowest rank) .. 1 + less + tied among the N - 1 other rows.  A slot holding
 * -1 (empty) or i itself gets less = tied = -1.  The threshold d(i, n) is summed by a gather launch in the order of the
 * tile contraction, so it is bit for bit the value the tile pass produces for that pair: a row never counts its
 * neighbour's own rounding as a tie, and the k nearest rows in A itself get less = 0 .. k - 1 exactly (ties apart).
 * Counts are combined over the column chunks with integer atomics: bitwise reproducible, independent of the chunking.
 * An index outside [0, N) other than -1 is NOT an error of this entry: no row is read for it and the slot leaves as an
 * empty one (-1, -1); the host wrapper ops.knn_ranks refuses such a table with ValueError before the call.
 * Both outputs are written in full (no need to clear them).  1 <= k <= 64 (more: VSOM_EUNSUPPORTED), 2 <= N <= 2^31 - 129,
 * lda >= D >= 1, metric as vsom_umap_knn; 16-byte row loads under the conditions of vsom_knn_query, element-wise
 * otherwise (operands of 4 GB or more take the element-wise loads).  Workspace: vsom_knn_ranks_workspace_bytes(N, k)
 * (host arithmetic; 0 for a non-positive size): the N squared norms, the N k thresholds and the N k neighbours as int32,
 * each rounded up to 256 bytes. */
size_t vsom_knn_ranks_workspace_bytes(long N, int k);
int vsom_knn_ranks(const float* A, long lda, long N, int D, int metric, const int64_t* nbr, int k, int32_t* less, int32_t* tied,
                   void* ws, size_t ws_bytes, vsom_stream_t stream);
/* Silhouette coefficient (Rousseeuw 1987; sklearn.metrics.silhouette_samples; vit_som_amd/silhouette.py; no counterpart
 * in the reference) of the rows of X [N, D] (row stride ldx) under labels int64 [N] in [0, n_clusters): the contraction
 * of vsom_knn_ranks with a summing epilogue.  Every distance d(i, j) is that of vsom_umap_knn, except that dot products
 * and squared norms are summed in segments of 128 k-values (each in the search's order, the segment sums added in ascending
 * order in fp32: shorter chains, a more accurate sum; for D <= 128 the value is bit for bit the search's, for every D
 * identical rows are at distance exactly 0 and a pair's value does not depend on its place in a tile).  It is
 * turned into fixed point, q = llrint((double)d * 2^(40 - e)), where 2^e is the smallest power of two > 4 sqrt(max
 * squared norm) (cosine: 4), found on the device, and added into S[i][labels[j]] (uint64, integer atomics).  Then in fp64
 *   a[i] = S[i][own] unit / (n_own - 1),  b[i] = min over the other non-empty clusters c of S[i][c] unit / n_c (the lowest
 *   c on a tie; nearest[i] = that c),  sil[i] = (b - a) / max(a, b),  unit = 2^(e - 40);
 * sil = 0 (a = 0) for a singleton cluster, sil = 0 where max(a, b) = 0, and with no other non-empty cluster sil = 0,
 * b = NaN, nearest = -1.  counts[c] = members of cluster c; cluster_mean[c] = mean of sil over them (NaN when empty);
 * score[0] = mean of sil over the counted rows; both means are exact integer sums of llrint(sil 2^40) divided once.
 * A row whose label is outside [0, n_clusters) gets sil = a = b = NaN and nearest = -1, is part of no sum, no count and
 * no bound: the other rows come out as if it were absent.  A pair adds nothing when one of its rows has a NaN or
 * overflowed squared norm or its distance is not below 2^e.  status int64 [4]: [0] rows with a label out of range,
 * [1] such refused distances (each ordered pair), [2] non-empty clusters, [3] singleton clusters.
 * All integer sums: every output is bitwise reproducible and bit for bit independent of the order of the rows and of the
 * launch's chunking.  a, b, nearest and cluster_mean may be NULL; every output given is written in full (no need to clear
 * it).  2 <= N <= 2^22 - 1 (more: VSOM_EUNSUPPORTED -- a row's sum of N values below 2^40 must stay below 2^63),
 * n_clusters >= 1, ldx >= D >= 1, metric VSOM_DIST_COSINE | VSOM_DIST_EUCLIDEAN; 16-byte row loads under the conditions
 * of vsom_knn_query, element-wise otherwise (operands of 4 GB or more take the element-wise loads).  Workspace:
 * vsom_silhouette_workspace_bytes(N, n_clusters) (host arithmetic; 0 for a non-positive size), 16-byte aligned; its first
 * N * n_clusters uint64 words are S, left there for the caller. */
size_t vsom_silhouette_workspace_bytes(long N, int n_clusters);
int vsom_silhouette(const float* X, long ldx, long N, int D, int metric, const int64_t* labels, int n_clusters, double* sil,
                    double* a, double* b, int64_t* nearest, int64_t* counts, double* cluster_mean, double* score,
                    int64_t* status, void* ws, size_t ws_bytes, vsom_stream_t stream);
/* The class vote over such lists, one wave per query: scores[i, c] (fp64) = the weights of query i's neighbours j with
 * bank_labels[idx[i, j]] == c, added in neighbour order j = 0 .. k-1; pred[i] = the first argmax (ties go to the
 * lowest class, as vsom_argmax_rows).  weights:
 *   VSOM_KNN_UNIFORM   1;
 *   VSOM_KNN_DISTANCE  sklearn's rule: 1 / d in fp64 from the stored fp32 distance; if any counted neighbour of the
 *                      query is at distance 0 those get 1 and the others 0;
 *   VSOM_KNN_SOFTMAX   exp(-(d - d_min) / temperature) in fp64, d_min the query's smallest counted distance and
 *                      temperature > 0 (else VSOM_EINVAL): the softmax weights up to a common factor per query (for
 *                      cosine the DINO-style exp(sim / T) vote).  The nearest counted neighbour weighs exactly 1, so
 *                      the scores neither overflow nor, at euclidean distances of latent width, all underflow to 0.
 * An entry with idx < 0 is skipped; an idx >= n_bank or a label outside [0, n_classes) is skipped and counted in
 * status[0]; a query left without a counted neighbour gets pred = -1 and is counted in status[1] (status int32 [2],
 * zeroed by the caller).  scores [Nq, n_classes] may be NULL.  k <= 64, n_classes <= 1024: else VSOM_EUNSUPPORTED. */
#define VSOM_KNN_UNIFORM 0
#define VSOM_KNN_DISTANCE 1
#define VSOM_KNN_SOFTMAX 2
int vsom_knn_vote(const int64_t* idx, const float* dist, long Nq, int k, const int64_t* bank_labels, long n_bank,
                  int n_classes, int weights, float temperature, int64_t* pred, double* scores, int* status,
                  vsom_stream_t stream);

/* ------------------------------------------------------------------ principal component analysis (pca.hip)
 * The kernels of a block subspace iteration on the covariance operator of X [N, D] (row stride ldx) with a basis kept as
 * ROWS, B [l, D] (sklearn's components_ layout); vit_som_amd/pca.py drives them, DESIGN.md section 4 has the algorithm;
 * no counterpart in the reference.  Limits of every entry: l <= 256 and l <= D, N >= 2 where N is given (else
 * VSOM_EUNSUPPORTED).  Scratch is a TYPED array with an element count, sized by a host-only query (0 for a non-positive
 * size); a count below the query or a null array is VSOM_EWORKSPACE, an array that is not 16-byte aligned VSOM_EALIGN,
 * both before any launch.  No floating-point atomics; every sum has one fixed order: all outputs are bitwise reproducible.
 *
 * vsom_pca_colstats: mean[c] (f32) = the column mean, summed in fp64 and rounded once; var[c] (fp64) = sum (x - mean[c])^2
 * / (N - 1) about that ROUNDED mean, in a second sweep.  The rows are split over vsom_pca_colstats_parts(N, D) / D
 * workgroup rows (at least two workgroups per CU at the benchmark's shape), the per-split fp64 partials added in split
 * order.  part: vsom_pca_colstats_parts(N, D) doubles. */
long vsom_pca_colstats_parts(long N, int D);
int vsom_pca_colstats(const float* X, long ldx, long N, int D, float* mean, double* var, double* part, long n_part,
                      vsom_stream_t stream);
/* Floats of slab space of vsom_pca_project (which = 0) and vsom_pca_backproject (which = 1): the reduction splits (a
 * function of the shape alone) times the output size. */
long vsom_pca_slabs(long N, int D, int l, int which);
/* Y [N, l] (row stride ldy) = (X - mean) B^T diag(scale): the hot kernel of transform and half of a pass.  mean [D] and
 * scale [l] may be NULL (no centring / no scaling; scale carries 1 / sqrt(explained variance) for whitening).  Exact-f32
 * matrix cores (v_mfma_f32_32x32x2_f32), both operands k-contiguous; the mean is subtracted from each X tile between the
 * global load and the LDS store, and only from elements inside the matrix.  The reduction over D is split, per-split
 * slabs are added in split order.  16-byte loads when D % 4 == 0 and X, B, mean and their strides are 16-byte aligned,
 * element-wise otherwise; operands of 4 GB or more take the element-wise loads (from 0xFFFF0000 bytes, counted from the
 * base to the end of the last row; no error).  Y is written through a plain pointer at any pitch. */
int vsom_pca_project(const float* X, long ldx, long N, int D, const float* mean, const float* B, long ldb, int l,
                     const float* scale, float* Y, long ldy, float* slabs, long n_slabs, vsom_stream_t stream);
/* Zt [l, D] (row stride ldz) = Y^T (X - mean): the other half of a pass; both operands k-strided (the shape of a weight
 * gradient), the reduction over the N rows split the same way.  16-byte loads additionally want ldy % 4 == 0; operands
 * of 4 GB or more take the element-wise loads, as in vsom_pca_project. */
int vsom_pca_backproject(const float* Y, long ldy, const float* X, long ldx, long N, int D, const float* mean, int l, float* Zt,
                         long ldz, float* slabs, long n_slabs, vsom_stream_t stream);
/* G [l, l] = Zt Zt^T and, when B (and H) are given, H [l, l] = B Zt^T: products and sums in fp64, each entry one
 * fixed-order sum over D (G is symmetric bit for bit); dense row-major outputs, no workspace. */
int vsom_pca_gram(const float* Zt, long ldz, const float* B, long ldb, int l, int D, double* G, double* H, vsom_stream_t stream);
/* Bout [l_out, D] (row stride ldo) = T Zt with T fp64 [l_out, l_in] dense on the device: fp64 accumulation over the rows
 * of Zt in ascending order, one rounding to f32.  Bout may not overlap Zt (VSOM_EINVAL). */
int vsom_pca_rotate(const double* T, int l_out, int l_in, const float* Zt, long ldz, int D, float* Bout, long ldo,
                    vsom_stream_t stream);
/* Xout [M, D] (row stride ldo) = (Y diag(scale)) B + mean, Y [M, l]; scale and mean may be NULL: inverse_transform and the
 * linear initialisation of the SOM.  f32 fma chain over the l components in ascending order; bound by the output store.
 * M <= 262140 rows per call. */
int vsom_pca_reconstruct(const float* Y, long ldy, long M, int l, const float* scale, const float* B, long ldb, int D,
                         const float* mean, float* Xout, long ldo, vsom_stream_t stream);

/* ------------------------------------------------------------------ Kohonen's batch map (batch_som.hip)
 * One epoch of the batch SOM at radius sigma (SOMLayer.fit_batch drives it, DESIGN.md section 4 has the algorithm; no
 * counterpart in the reference): the per-unit sums of the rows each unit won, then every prototype as the neighbourhood-
 * weighted mean of those sums.  Scratch is a typed array with an element count, sized by a host-only query (0 for a size
 * the entry refuses); a count below the query or a null array is VSOM_EWORKSPACE before any launch.  No floating-point
 * atomics; every sum has one fixed order: all outputs are bitwise reproducible.
 *
 * vsom_som_batch_accumulate: counts[c] (int64) = the rows whose bmu is c, sums[c][d] (fp64, dense [K, D]) = the sum over
 * those rows, in ASCENDING ROW INDEX, of (double)X[i][d] * (double)inv_norm[i] (inv_norm may be NULL: the rows themselves).
 * `order` [N] is the stable sort permutation of bmu (order[j] = the row at sorted position j; torch.sort(stable=True)
 * gives it).  accumulate = 0 overwrites sums and counts (units without rows get zeros), accumulate = 1 continues every
 * chain from what they hold: cutting the rows into several calls changes no bit, and the result equals a sequential fp64
 * loop over the rows.  A bmu outside [0, K) or an order entry outside [0, N) adds one to *bad (int, zeroed by the caller)
 * and is never dereferenced; its row is left out.  16-byte loads when D % 4 == 0, ldx % 4 == 0 and X is 16-byte aligned,
 * element-wise otherwise.  seg: vsom_som_batch_accumulate_parts(K) = K + 1 int64.  K <= 65535 (else VSOM_EUNSUPPORTED). */
long vsom_som_batch_accumulate_parts(int K);
int vsom_som_batch_accumulate(const float* X, long ldx, long N, int D, const int64_t* bmu, const int64_t* order,
                              const float* inv_norm, int K, double* sums, int64_t* counts, int accumulate, int* bad, int64_t* seg,
                              long n_seg, vsom_stream_t stream);
/* vsom_som_batch_update: W_out[k] (f32, row stride ldw) = sum_c h(k,c) sums[c] / sum_c h(k,c) counts[c] over the units with
 * counts[c] > 0, h(k,c) = exp(-(d2(k,c) - m_k) / (2 sigma^2)), d2 the squared distance of grid_positions [K, 2], m_k the
 * smallest d2(k,c) among the units with hits: the largest weight of every row is exactly 1, so a unit far from every hit
 * at a small radius is the mean of its nearest hit units instead of 0 / 0.  m_k and the denominators in fp64 (pre-pass);
 * the numerator on the exact-f32 matrix cores, the weights generated from the positions (exponent in fp64, rounded once),
 * sums rounded to f32 as loaded, the reduction over c in ascending order inside one workgroup.  normalize != 0: every row
 * is L2-normalised afterwards (x / max(|x|, 1e-12)).  No unit with hits at all: W_out = 0.  sigma <= 0, not finite, or so
 * extreme that 1 / (2 sigma^2) is 0 or infinite: VSOM_EINVAL.  part: vsom_som_batch_update_parts(K) = 4 K doubles. */
long vsom_som_batch_update_parts(int K);
int vsom_som_batch_update(const double* sums, const int64_t* counts, const float* grid_positions, int K, int D, double sigma,
                          int normalize, float* W_out, long ldw, double* part, long n_part, vsom_stream_t stream);

/* ------------------------------------------------------------------ linear probe (linear_probe.hip)
 * Multinomial logistic regression on frozen features (vit_som_amd/linear_probe.py drives it, DESIGN.md section 4 has the
 * algorithm; no counterpart in the reference).  The two passes over X of an iteration are vsom_pca_project (the logits) and
 * vsom_pca_backproject (the gradient); the entries below never touch X.  Parameters are one fp64 vector theta = W [C, D]
 * row-major, then b [C] when there is an intercept.  2 <= C <= min(256, D) and N >= 2 (the contraction's limits), else
 * VSOM_EUNSUPPORTED.  Every sum has one fixed order (per-workgroup fp64 partials added in workgroup order), no
 * floating-point atomics: results are bitwise reproducible.  `part` buffers are scratch, sized by the matching query in
 * doubles; one that is NULL or too small is refused with VSOM_EWORKSPACE before any launch.
 *
 * vsom_probe_fold: B[c][d] (f32, row stride ldb) = A[c][d] * invstd[d], fp64 product rounded once -- the standardisation
 * folded into the weights (A = W) or into a search direction (A = P).  With W (fp64 [C, D], dense) also pen[3] =
 * {W.W, W.A, A.A} in fp64: the penalty along A is a quadratic in the step.  W and pen go together; part:
 * vsom_probe_fold_parts(C, D) doubles, needed with W only. */
long vsom_probe_fold_parts(int C, int D);
int vsom_probe_fold(const double* A, const double* invstd, int C, int D, float* B, long ldb, const double* W, double* pen,
                    double* part, long n_part, vsom_stream_t stream);
/* Doubles of scratch of vsom_probe_residual and vsom_probe_linesearch at this shape (host arithmetic; 0 outside the limits). */
long vsom_probe_parts(long N, int C);
/* vsom_probe_residual: for the logits Z [N, C] (f32, row stride ldz), the intercept b (fp64 [C], nullable = 0) and labels
 * y (int64 [N]): R[i] (f32, row stride ldr) = softmax(Z[i] + b) - onehot(y[i]), computed in fp64 with the row maximum
 * subtracted and rounded once; loss[0] (fp64) = sum_i CE_i = sum_i log sum_c exp(z_ic) - z_i,y[i]; gb[c] (fp64) = the column
 * sums of the ROUNDED R.  pred (int64 [N], nullable): the first index of the row maximum; prob (fp64 [N, C] dense, nullable):
 * the softmax.  A label outside [0, C) is counted in status[0] (int32, the caller zeroes it) and never used as an index:
 * its row of R is zero and it adds nothing to loss and gb (pred and prob are written all the same). */
int vsom_probe_residual(const float* Z, long ldz, long N, int C, const double* b, const int64_t* y, float* R, long ldr, double* loss,
                        double* gb, int64_t* pred, double* prob, int* status, double* part, long n_part, vsom_stream_t stream);
/* vsom_probe_linesearch: phi[j] (fp64, j < nsteps <= 16) = sum_i CE(Z[i] + a_j Zp[i] + b + a_j pb, y[i]) with
 * a_j = alpha0[0] * 2^-j (alpha0 on the device), every logit fma(a_j, Zp, Z) + fma(a_j, pb, b) in fp64: the whole ladder in
 * one launch, no pass over X.  Z and Zp share the row stride ldz; b and pb go together (nullable).  Rows whose label is
 * outside [0, C) add nothing. */
int vsom_probe_linesearch(const float* Z, const float* Zp, long ldz, long N, int C, const double* b, const double* pb,
                          const int64_t* y, const double* alpha0, int nsteps, double* phi, double* part, long n_part,
                          vsom_stream_t stream);
/* vsom_probe_step: the Armijo choice, made on the device, and the move.  F(a) = phi(a) / N + lam / 2 (pen[0] + 2 a pen[1] +
 * a^2 pen[2]), F(0) likewise from f0[0] (the summed CE at Z); the largest a_j = alpha0[0] 2^-j with
 * F(a_j) <= F(0) + c1 a_j gtp[0] is alpha.  Then Z += alpha Zp (fp64 fma, rounded once), theta += alpha p, s_new = alpha p
 * (n elements each).  rec[12 .. 15] = {alpha, status, F(alpha), j}; status 1: no step of the ladder passes, 2: gtp >= 0 --
 * alpha = 0, Z and theta stay, s_new = 0.  phi, alpha0, f0, pen, gtp, rec: fp64 on the device; rec may be the state record
 * of the L-BFGS pieces (alpha0 = rec, gtp = rec + 1). */
int vsom_probe_step(const double* phi, int nsteps, const double* alpha0, const double* f0, const double* pen, const double* gtp,
                    double lam, double c1, float* Z, const float* Zp, long ldz, long N, int C, double* theta, const double* p,
                    double* s_new, long n, double* rec, vsom_stream_t stream);
/* vsom_probe_gradient: g[c D + d] = Zt[c][d] invstd[d] / N + lam theta[c D + d] from Zt = R^T (X - mean) (f32 [C, D], row
 * stride ldz), and with intercept != 0 g[C D + c] = gb[c] / N; y_new = g - g_prev (both nullable, together).  fp64. */
int vsom_probe_gradient(const float* Zt, long ldz, const double* invstd, const double* theta, const double* gb, int C, int D,
                        int intercept, long N, double lam, const double* g_prev, double* g, double* y_new, vsom_stream_t stream);

/* ------------------------------------------------------------------ L-BFGS pieces (linear_probe.hip)
 * The limited-memory BFGS direction in dot-product-matrix form, for any smooth objective over fp64 vectors of length n:
 * the pieces know nothing of the probe.  The caller holds S [m, n] and Y [m, n] (ring slots, dense), the gradient g, the
 * newest pair s_new = x_k+1 - x_k, y_new = g_k+1 - g_k, and `state`: vsom_lbfgs_state_doubles(m) doubles, ZEROED before
 * the first call.  m <= 16.  state[0 .. 16) is the record
 *   {alpha0, g.p, g.g, max |g|, pairs held, pairs skipped, pair accepted, its slot, next slot, -, -, -, 4 words for the caller},
 * then the Gram matrix of the 2 m + 1 vectors (S slots, Y slots, g) and the 2 m + 1 coefficients of the direction.
 * Per iteration:
 *   vsom_lbfgs_dots     dots[k (2 m + 3) + v] = (s_new, y_new, g)[k] . v over the vectors (S slots held, Y slots held, g,
 *                       s_new, y_new), dots[3 (2 m + 3)] = max |g|: ONE pass over the vectors, fp64 per-workgroup partials added
 *                       in workgroup order.  has_new = 0: no pair (the first iteration, or a restart): g.g and max |g| only.
 *                       dots: 3 (2 m + 3) + 1 doubles; part: vsom_lbfgs_parts(n, m) doubles.
 *   vsom_lbfgs_coeff    one small workgroup: the pair is accepted into the next ring slot when s.y > 0 (else counted as skipped),
 *                       its dot products enter the Gram matrix, and the two-loop recursion runs on coefficients.
 *                       has_new = 0 empties the history (p = -g).  alpha0 = 1, or min(1, 1 / |g|) without history.
 *   vsom_lbfgs_combine  an accepted pair is copied into its slot, and p = sum_j coefficient_j vector_j (one fma chain per
 *                       element: S slots, Y slots, g). */
long vsom_lbfgs_state_doubles(int m);
long vsom_lbfgs_parts(long n, int m);
int vsom_lbfgs_dots(const double* S, const double* Y, const double* g, const double* s_new, const double* y_new, long n, int m,
                    int has_new, const double* state, double* dots, double* part, long n_part, vsom_stream_t stream);
int vsom_lbfgs_coeff(const double* dots, int m, int has_new, double* state, vsom_stream_t stream);
int vsom_lbfgs_combine(double* S, double* Y, const double* g, const double* s_new, const double* y_new, long n, int m,
                       const double* state, double* p, vsom_stream_t stream);

/* ------------------------------------------------------------------ t-SNE (tsne.hip)
 * scikit-learn's TSNE with an exact all-pairs repulsion (vit_som_amd/tsne.py drives it and states the algorithm, DESIGN.md
 * section 4 has the bounds; no counterpart in the reference).  Two components only: a third changes the degrees of freedom
 * and with them the kernel of q.  No floating-point atomics; every sum has one fixed order: all outputs are bitwise
 * reproducible.  Caller-owned fp64 arrays with an element count are sized by a host-only query (0 for a non-positive
 * size); a count below the query or a null array is VSOM_EWORKSPACE before any launch.
 *
 * vsom_tsne_affinities: the conditional P of every row from its neighbour table, sklearn's _binary_search_perplexity in
 * fp64, rule for rule.  The row's values are knn_dist[i][first .. first + k_eff) (f32, row stride ldk: first = 1 skips the
 * self slot of vsom_umap_knn); square != 0 squares them first, in f32 with one rounding, as sklearn squares its euclidean
 * distances (cosine distances are used as they are).  With d_j the fp64 image of those values: beta = 1; at most 100 steps
 * of  e_j = exp(-d_j beta), S = sum_j e_j (ascending j; S = (double)1e-8f when it is 0), H = log S + beta sum_j d_j (e_j / S);
 * stop when |H - log (double)(float)perplexity| <= (double)1e-5f; H too large: beta_min = beta and beta doubles while
 * beta_max is infinite, else the midpoint; H too small: the mirror image with halving.  Outputs: P[i][j] = e_j / S (fp64,
 * dense [N, k_eff]) and beta[i] at the LAST EVALUATED beta (after 100 steps without a stop: the hundredth).  A row with a
 * distance that is NaN, infinite or negative, a square that overflows, or (knn_idx given, same layout, nullable) an empty
 * slot (index < 0) adds one to status[0] (int32, zeroed by the caller) and is not evaluated: its P and beta are not
 * written.  1 <= k_eff <= 63 (more: VSOM_EUNSUPPORTED), ldk >= first + k_eff. */
int vsom_tsne_affinities(const float* knn_dist, const int64_t* knn_idx, long ldk, long N, int k_eff, int first, int square,
                         double perplexity, double* P, double* beta, int32_t* status, vsom_stream_t stream);
/* vsom_tsne_repulsion: for Y f32 [N, 2] (dense, 16-byte aligned, finite) and every row i, over ALL j != i with
 * q_ij = 1 / (1 + |y_i - y_j|^2):  rep[i] (fp64 [N, 2]) = sum_j q_ij^2 (y_i - y_j),  sumq[i] (fp64 [N]) = sum_j q_ij, and
 * zpart[b] (fp64) = the sum of sumq over rows [64 b, 64 b + 64) in ascending row order; Z = sum_i sumq[i] is the sum of
 * zpart (vsom_tsne_step adds it).  zpart: vsom_tsne_repulsion_parts(N) = ceil(N / 64) doubles.
 * Tiled all-pairs: a workgroup owns 64 rows and walks the columns in tiles of 1024 staged in LDS; every lane of a wave
 * reads the same column (broadcast reads).  The pair (i, i) is excluded by index: coincident points are legal and count
 * with q = 1.  The symmetry (i, j) / (j, i) is not used.  The differences are taken in f32 before squaring; the reciprocal
 * is v_rcp_f32 (1 ulp).
 * Order of the sums: the columns are cut into chunks of 64; a chunk's terms are added in f32 in ascending column order;
 * chunk c belongs to group c mod 16, a group adds its chunks in fp64 in ascending order, the 16 groups are added in fp64
 * in ascending order.  Error of Z (all terms are positive, so relative errors carry through): a term q is within 8 * 2^-24
 * of its value (two differences, a sum of two squares, 1 +, a reciprocal of 1 ulp) and an f32 chain of 64 positive terms
 * within 63 * 2^-24, so every chunk, every sumq[i] and Z are within (71 * 2^-24 + N * 2^-53) relative = 4.3e-6 of the
 * exact sums, whatever N: the fp64 part at N = 60 000 (3.6e9 terms, 5.6e7 chunks) is 7e-12.  rep's terms have both signs:
 * its error is bounded by the same factor times sum_j q^2 |y_i - y_j|.
 * N < 2^31 - 1 (else VSOM_EUNSUPPORTED). */
long vsom_tsne_repulsion_parts(long N);
int vsom_tsne_repulsion(const float* Y, long N, double* rep, double* sumq, double* zpart, long n_zpart, vsom_stream_t stream);
/* vsom_tsne_step: one iteration from the outputs of vsom_tsne_repulsion at Y_in.  The joint P is a symmetric CSR (indptr
 * int64 [N + 1], indices int64, data FP64, unexaggerated).  For every row i, all in fp64 and from the iteration-start Y_in
 * (f32 [N, 2]; Y_out must not alias it):
 *   Z = sum zpart (64 ascending segments, added in ascending order: the same bits in every workgroup)
 *   attraction_i = sum_e exaggeration p_e q_e (y_i - y_j),  q_e = 1 / (1 + |y_i - y_j|^2) (edge l of the row belongs to lane
 *                  l mod 16; a lane adds its edges in ascending order, the 16 lanes meet in a butterfly)
 *   grad_i = 4 (attraction_i - rep[i] / Z)
 * and per component, with update and gains f32 [N, 2] updated in place (sklearn's rule):
 *   gains = gains + 0.2f if (double)update * grad < 0 else gains * 0.8f, then max(gains, 0.01f)          (f32)
 *   update = (float)(momentum (double)update - (learning_rate (double)gains) grad)                       (one rounding)
 *   Y_out = Y_in + update                                                                               (f32)
 * record != 0: part[2 w] = the KL over the edges of workgroup w's 16 rows, sum_e P_e log(max(P_e, eps) / max(q_e / Z, eps))
 * with P_e = exaggeration p_e and eps = 2^-52 as sklearn reports it, part[2 w + 1] = their sum of |grad_i|^2; the caller
 * adds the vsom_tsne_step_parts(N) / 2 pairs.  record == 0 skips the logarithms and leaves part alone.  An index outside
 * [0, N) is never dereferenced (its edge is left out).  part: vsom_tsne_step_parts(N) = 2 ceil(N / 16) doubles; zpart as
 * above.  N < 2^31 - 1. */
long vsom_tsne_step_parts(long N);
int vsom_tsne_step(const int64_t* indptr, const int64_t* indices, const double* data, const float* Y_in, float* Y_out,
                   float* update, float* gains, long N, const double* rep, const double* zpart, long n_zpart, double exaggeration,
                   double momentum, double learning_rate, int record, double* part, long n_part, vsom_stream_t stream);

/* SOMLayer.som_loss(weights, distances) = mean(weights * distances) for ARBITRARY weights (som_layer.py:137-142):
   loss_sum <- sum_ik weights[i,k] dist[i,k]; with coef/row_dot/col_dot given, also the backward coefficients of
   grad_scale * that sum w.r.t. the distances' inputs (what vsom_som_bwd consumes) -- with weights = an upstream
   gradient dL/d dist this is the autograd of SOMLayer.forward itself.  Workspace: vsom_som_neigh_workspace_bytes. */
int vsom_som_weighted_loss(const float* dist, const float* weights, const float* inv_nx, const float* inv_nw,
                           float grad_scale, float* loss_sum, float* coef, float* row_dot, float* col_dot, int B, int K,
                           int distance, void* ws, size_t ws_bytes, vsom_stream_t stream);

/* Cosine BMU pass as a reduced-precision contraction + exact re-rank; replaces
   F.normalize x 2 + matmul + argmin of som_layer.py:119-122, 83-89 in one pass over X and W:
   stage 1 = X W^T on the bf16 matrix cores from a two-piece round-to-nearest split (three products; |error of
   the normalised dot| <= 3 * 2^-16) + the squared row norms of X and W; stage 2 = inv_nx / inv_nw
   (1 / max(|row|, 1e-12)), dist, and bmu = first argmin after every prototype within 2e-4 of the approximate
   minimum has been re-ranked with an exact (fp64-accumulated) dot product, whose distance also replaces the
   approximate one in dist: bmu == argmin(dist) exactly.  K <= 2048; rows 16-byte aligned: X and W 16-byte aligned, L and
   ldx multiples of 4.  vsom_bmu_cosine_x3_dots answers VSOM_EALIGN to anything else (the caller then runs the exact form);
   vsom_bmu_cosine_x3_finalize, whose re-rank reads the rows of X and W 16 bytes at a time, answers VSOM_EALIGN to a
   misaligned X or W and VSOM_EINVAL to an L or ldx that stage 1 would have refused.  X (from its base to the end of its last
   row, at pitch ldx) and W below 4 GB (0xFFFF0000 bytes): stage 1 reads them as buffer resources and has no other form;
   vsom_bmu_cosine_x3_dots and vsom_bmu_cosine_x3_finalize alike answer VSOM_EUNSUPPORTED to a larger operand. */
size_t vsom_bmu_cosine_x3_workspace_bytes(int B, int K, int L);
int vsom_bmu_cosine_x3_dots(const float* X, long ldx, const float* W, int B, int K, int L, void* ws, size_t ws_bytes,
                            vsom_stream_t stream);
int vsom_bmu_cosine_x3_finalize(const float* X, long ldx, const float* W, const void* ws, size_t ws_bytes, float* dist,
                                int64_t* bmu, float* inv_nx, float* inv_nw, int* reranked, int B, int K, int L,
                                vsom_stream_t stream);

/* The same pass on PRE-SPLIT operands ("plane images"): the two-piece bf16 split is taken out of the contraction and done
   once per operand -- for the prototypes by the optimizer step that rewrites them anyway (vsom_adamw_step_planes), for the
   samples by vsom_bmu_planes_from -- so that the contraction is LDS-DMA -> ds_read -> MFMA with no VALU in its loop.
   A plane buffer (vsom_bmu_planes_bytes(R, L) bytes, 16-byte aligned) holds, for an operand [R, L]: the fragment image
   (per 16-deep k step and 32-row block the two planes as 1 KB MFMA fragments, rows >= R and k >= L zero) followed by the
   rows' squared-norm partials.  The caller owns validity: a plane buffer describes the operand as it was when written.
   Covered shapes: vsom_bmu_cosine_x3_planes_supported (B >= 192, L % 8 == 0, K <= 2048, images < 2 GB); slabs, and
   therefore dist / bmu, are those of vsom_bmu_cosine_x3_dots bit for bit (norms: last-bit differences).
   Alignment: vsom_bmu_planes_from wants src 16-byte aligned and ld % 4 == 0 (VSOM_EINVAL otherwise) and, like
   vsom_adamw_step_planes, a 16-byte aligned plane buffer (VSOM_EWORKSPACE); vsom_bmu_cosine_x3_planes_dots refuses a
   misaligned plane buffer with VSOM_EINVAL; vsom_bmu_cosine_x3_planes_finalize reads the rows of X and W 16 bytes at a time
   in its re-rank: X and W 16-byte aligned (VSOM_EALIGN), ldx % 4 == 0 (VSOM_EINVAL), and X and W below 4 GB as for
   vsom_bmu_cosine_x3_finalize (VSOM_EUNSUPPORTED).  An image of 2 GB or more (it is one buffer resource) is refused by
   every entry that takes a plane buffer with VSOM_EUNSUPPORTED; the pitch of src has no limit (plain pointers).
   Same reference lines as above (som_layer.py:119-122, 83-89); the AdamW variant replaces vit_som.py:146-151. */
size_t vsom_bmu_planes_bytes(int R, int L);
int vsom_bmu_planes_from(const float* src, long ld, int R, int L, void* planes, size_t planes_bytes, vsom_stream_t stream);
/* vsom_adamw_step over the arena of n elements (same arguments, bitwise the same update) that also writes the plane
   buffer of the [R, L] parameter at element offset slice_off (a multiple of 256) from its UPDATED values.  p, g, m and v
   16-byte aligned, as for vsom_adamw_step (VSOM_EALIGN). */
int vsom_adamw_step_planes(float* p, const float* g, float* m, float* v, const float* wd_per_chunk, long n, float lr,
                           float beta1, float beta2, float eps, int step, float grad_scale, int adamw, long slice_off,
                           int R, int L, void* planes, size_t planes_bytes, vsom_stream_t stream);
int vsom_bmu_cosine_x3_planes_supported(int B, int K, int L);
size_t vsom_bmu_cosine_x3_planes_workspace_bytes(int B, int K, int L);
int vsom_bmu_cosine_x3_planes_dots(const void* xplanes, const void* wplanes, int B, int K, int L, void* ws, size_t ws_bytes,
                                   vsom_stream_t stream);
int vsom_bmu_cosine_x3_planes_finalize(const float* X, long ldx, const float* W, const void* xplanes, const void* wplanes,
                                       const void* ws, size_t ws_bytes, float* dist, int64_t* bmu, float* inv_nx, float* inv_nw,
                                       int* reranked, int B, int K, int L, vsom_stream_t stream);

/* Which of the three forms above a caller of the cosine BMU pass should run for B sample rows of stride ldx against K
   prototypes of L elements, under the current GEMM mode ("Which kernel runs": Cosine BMU pass):
   VSOM_BMU_EXACT (vsom_bmu_cosine_*, after the two row-norm passes), VSOM_BMU_X3 (vsom_bmu_cosine_x3_*) or VSOM_BMU_X3_PLANES
   (vsom_bmu_cosine_x3_planes_*).  flags bit 0: X and W are 16-byte aligned; bit 1: the caller can supply plane images.  Pure host
   arithmetic, the same plan the entry points take their grids and workspace sizes from.  VSOM_EINVAL on a non-positive
   shape. */
#define VSOM_BMU_EXACT 0
#define VSOM_BMU_X3 1
#define VSOM_BMU_X3_PLANES 2
int vsom_bmu_cosine_form(int B, int K, int L, long ldx, int flags);

/* ------------------------------------------------------------------ data: the input side of a step (augment.hip)
 * A data set lives on the device as uint8 [N, C, H, W] (C 1 or 3, square, H <= 64).  vsom_augment_plan writes one row of
 * VSOM_AUGMENT_PARAMS int32 per sample: {i1, j1, h1, w1,  i2, j2, h2, w2 (h2 = 0: no second crop),  flip,
 * erase top, left, h, w (h = 0: none),  0, 0, 0}, drawn with Philox4x32-10 from (seed, epoch, index[b]) alone (index[b]
 * clamped into [0, N), N = rows of the data set) -- counter
 * (block, index, 0, epoch), key seed -- so a sample's augmentation does not depend on its place in a batch, the batch size or
 * the rank count.  Boxes: the loop-free RandomResizedCrop draw of tools/utils.py:93-113 (area share U(scale0, scale1),
 * aspect exp(U(log_ratio0, log_ratio1)), Python rounding, clamped to [1, size]), the second on the S x S result of the
 * first; flip: one Bernoulli(flip_p); erase: timm RandomErasing's draw with probability erase_p (ten attempts of
 * area U(0.02, 1/3) S^2, aspect exp(U(log 0.3, log 1/0.3)), accepted when h < S and w < S).  params is written a row (64
 * bytes) at a time and must be 16-byte aligned (VSOM_EALIGN), here and wherever a batch entry below reads it. */
#define VSOM_AUGMENT_PARAMS 16
int vsom_augment_plan(const int64_t* index, long N, int B, int H, int S, double scale0, double scale1, double log_ratio0,
                      double log_ratio1, int two_stage, double scale2_0, double scale2_1, double log_ratio2_0,
                      double log_ratio2_1, double flip_p, double erase_p, uint64_t seed, int epoch, int32_t* params,
                      vsom_stream_t stream);
/* out[b] (fp32 [B, C, S, S], 16-byte aligned) = the transform of data/data.py:287-313 applied to src[index[b]]:
 * crop box 1 -> R x R with PIL's 8-bit antialiased bicubic (Image.crop(...).resize(..., BICUBIC) bit for bit: 22-bit
 * fixed-point coefficients, horizontal pass first, 8-bit intermediate); with R == S optionally crop box 2 of that -> S x S
 * again (the image stays in LDS); the S x S window at (off, off) of the result; horizontal flip; level / 255;
 * (v - mean[c]) / std[c] (two true fp32 divides); inside the erase box a standard normal per element (Philox counter
 * (element / 4, index, 1, epoch), Box-Muller in fp32).  params = NULL: the whole image, no flip, no erase -- the evaluation
 * transform with R = int(S / 0.875), off = round((R - S) / 2), or identity geometry with R = S = H.  out_u8 (nullable,
 * [B, C, S, S], 4-byte aligned) receives the 8-bit image before normalisation.  mean, std: C floats on the device.
 * S <= 64, S <= R <= 73, H <= 4 S.  An index outside [0, N) is clamped into it, by both entries alike (N = rows of the
 * data set), so plan, noise and pixels still belong to one row; a box outside its image is moved inside.  out and params
 * not 16-byte aligned, or out_u8 not 4-byte aligned: VSOM_EALIGN. */
int vsom_augment_batch(const unsigned char* src, long N, int C, int H, int W, const int64_t* index, const int32_t* params,
                       int B, int S, int R, int off, const float* mean, const float* std, uint64_t seed, int epoch,
                       float* out, unsigned char* out_u8, vsom_stream_t stream);

/* RandAugment and timm's rand-m9 auto-augment (data/data.py:288-301): the training transform with both policies.
 * vsom_randaug_plan writes a second record of VSOM_RANDAUG_PARAMS int32 per sample (16-byte aligned rows), drawn with
 * Philox4x32-10 under stream 2 -- counter (block, index, 2, epoch), key seed -- so no draw of vsom_augment_plan moves:
 *   word 0       flip 1: RandomHorizontalFlip(flip1_p), applied before the second crop
 *   word 1       flip 2: timm's flip (probability 1/2), applied after the second crop
 *   words 2-5    the policy's pick for slots 0 .. 3 (index into torchvision's 14 ops / timm's 15 ops; -1: stage empty)
 *   word 6       bit t set: timm slot t is applied (each with probability 1/2);  word 7: 0
 *   words 8 + 16 s .. 23 + 16 s, s = 0 .. 3: op slot s (0, 1: the torchvision stage; 2, 3: the timm stage)
 *     +0   primitive: 0 none, 1 affine NEAREST, 2 affine BICUBIC, 3 brightness, 4 color, 5 contrast, 6 sharpness,
 *          7 posterize, 8 solarize, 9 solarize-add (threshold 128), 10 invert, 11 autocontrast, 12 equalize
 *     +1   integer parameter: bits kept (posterize, 0 .. 8), threshold (solarize, 0 .. 256), addend (solarize-add)
 *     +2   fp32 blend factor of the four enhance primitives (bit pattern)
 *     +3   fill of the affine primitives: R | G << 8 | B << 16 (one channel: the low byte)
 *     +4 .. +15  six doubles a0 .. a5: the inverse map (x_in, y_in) = (a0 x + a1 y + a2, a3 x + a4 y + a5) as
 *          Image.transform(size, AFFINE, data) takes it
 * Words 2-7 are for the reader of a record; vsom_augment_batch_ra reads words 0, 1 and the slots only.
 * torchvision stage, randaug_n (0 .. 2) slots: one of {Identity, ShearX, ShearY, TranslateX, TranslateY, Rotate, Brightness,
 * Color, Contrast, Sharpness, Posterize, Solarize, AutoContrast, Equalize} at magnitude bin 9 of 31 (shear 0.09, translate
 * int(150/331 S 0.3) px, rotate 9 degrees, enhance 1 +- 0.27, 7 bits, threshold 178.5), signed ones negated with
 * probability 1/2; NEAREST, fill fill_tv.  timm stage (autoaugment != 0), 2 slots: one of {AutoContrast, Equalize, Invert,
 * Rotate, PosterizeIncreasing, SolarizeIncreasing, SolarizeAdd, Color, Contrast, Brightness, SharpnessIncreasing, ShearX,
 * ShearY, TranslateXRel, TranslateYRel} at m = clamp(N(9, 0.5), 0, 10) (rotate 3 m degrees, shear 0.03 m, translate
 * 0.045 m S px, enhance max(0.1, 1 +- 0.09 m), 4 - int(0.4 m) bits, threshold 256 - int(25.6 m), addend min(128, int(11 m)));
 * BICUBIC, fill fill_timm.  Rotations follow Image.rotate about (S / 2, S / 2).  fill_*: R | G << 8 | B << 16.  ra not
 * 16-byte aligned: VSOM_EALIGN. */
#define VSOM_RANDAUG_PARAMS 72
int vsom_randaug_plan(const int64_t* index, long N, int B, int S, int randaug_n, int autoaugment, double flip1_p, uint32_t fill_tv,
                      uint32_t fill_timm, uint64_t seed, int epoch, int32_t* ra, vsom_stream_t stream);
/* vsom_augment_batch with R = S, off = 0 and the record `ra` ([B, VSOM_RANDAUG_PARAMS], 16-byte aligned) between its
 * stages: crop 1 -> slots 0, 1 -> flip 1 -> crop 2 (params' h2 > 0) -> flip 2 -> slots 2, 3 -> level / 255, Normalize, erase.
 * params (required) gives the crop boxes and the erase box; its merged flip (word 8) is not read.  Every primitive is PIL's,
 * byte for byte: Image.transform(AFFINE) in 16.16 fixed point (NEAREST) or in doubles with coordinates accumulated pixel by
 * pixel (BICUBIC), ImageEnhance's fp32 blend with its degenerate images, ImageOps' tables.  A slot that is not a record
 * the plan would write is made safe, never refused (the records live on the device): an unknown primitive does nothing, the
 * integer parameter is clamped to 0 .. 256, NaN coefficients become 0 and others are clamped to +-16384, a NaN factor
 * becomes 1.  out, params and ra 16-byte aligned, out_u8 4-byte aligned (VSOM_EALIGN otherwise). */
int vsom_augment_batch_ra(const unsigned char* src, long N, int C, int H, int W, const int64_t* index, const int32_t* params,
                          const int32_t* ra, int B, int S, const float* mean, const float* std, uint64_t seed, int epoch,
                          float* out, unsigned char* out_u8, vsom_stream_t stream);

/* ------------------------------------------------------------------ data: image sets of varying size (augment_ragged.hip)
 * The set is one flat uint8 buffer `data` of data_bytes bytes: image n is planar [C][H_n][W_n] at byte offsets[n] (int64,
 * a multiple of 16), with shapes[n] = {H_n, W_n} (int32 [N, 2]); C is 1 or 3 for the whole set and max_h, max_w bound every
 * side (at most 2048).  The transform is vsom_augment_plan's and vsom_augment_batch's -- the same plan row, Philox counters,
 * PIL resampler and output stage -- for outputs up to S = 224 and crops of up to 8 x their output side (33 taps).
 * vsom_augment_plan_ragged: vsom_augment_plan with box 1 drawn on the sample's own H_n x W_n.  On a table whose rows are
 * all (H, H) it writes what vsom_augment_plan(H) writes, bit for bit.  params 16-byte aligned, shapes 4-byte aligned
 * (VSOM_EALIGN otherwise). */
int vsom_augment_plan_ragged(const int64_t* index, const int32_t* shapes, long N, int B, int S, double scale0, double scale1,
                             double log_ratio0, double log_ratio1, int two_stage, double scale2_0, double scale2_1,
                             double log_ratio2_0, double log_ratio2_1, double flip_p, double erase_p, uint64_t seed, int epoch,
                             int32_t* params, vsom_stream_t stream);
/* Bytes of the 8-bit [B, C, S, S] image between the two training launches (16-byte aligned; one buffer serves every batch
 * of a stream). */
size_t vsom_augment_ragged_scratch_bytes(int B, int C, int S);
/* out[b] (fp32 [B, C, S, S], 16-byte aligned) = the transform applied to image index[b].
 * Training (params != NULL, R == S): crop box 1 of the H_n x W_n image -> S x S into `scratch`; box 2 of that (h2 > 0; else the
 * image as it is) -> S x S; flip, level / 255, Normalize, erase as vsom_augment_batch does them.  Two launches.
 * Evaluation (params == NULL): torchvision's Resize(R) of a rectangle -- the shorter side becomes R, the longer
 * int(R * long / short) (a double division, truncated) -- then CenterCrop(S) at top = rint((Rh - S) / 2.0), left likewise
 * (half to even), level / 255, Normalize.  Only the S x S window of the resize is computed.  One launch, no scratch.
 * Every resize is Image.crop(box).resize(size, BICUBIC) byte for byte: horizontal pass first, 8-bit intermediate, taps stop
 * at the box.  On a set whose images are all H x H, H <= 64, out and out_u8 equal vsom_augment_batch's bit for bit.
 * Limits (checked before any launch): S <= 224, R <= 256, C 1 or 3, max_h, max_w <= 2048 and <= 8 S (training) or 8 R
 * (evaluation); data, out, params, scratch 16-byte aligned, out_u8 and shapes 4-byte aligned, offsets 8-byte aligned
 * (VSOM_EALIGN otherwise).
 * Tables on the device cannot be refused, so they are made safe: the index is clamped into [0, N), the shape into
 * [1, max_h] x [1, max_w], the offset so that the image lies inside data[0, data_bytes), every box inside its image.  A bad
 * table reads wrong pixels, never outside the buffer. */
int vsom_augment_batch_ragged(const unsigned char* data, size_t data_bytes, const int64_t* offsets, const int32_t* shapes, long N,
                              int C, int max_h, int max_w, const int64_t* index, const int32_t* params, int B, int S, int R,
                              const float* mean, const float* std, uint64_t seed, int epoch, void* scratch, size_t scratch_bytes,
                              float* out, unsigned char* out_u8, vsom_stream_t stream);

/* ------------------------------------------------------------------ Gaussian mixtures (gmm.hip)
 * The steps of sklearn.mixture.GaussianMixture (covariance_type "diag" and "spherical") that touch the data;
 * vit_som_amd/gmm.py drives them, DESIGN.md section 4 has the numerical form; no counterpart in the reference.  X is
 * f32 [N, D] with row stride ldx (any alignment, any D: 16-byte loads when D % 4 == 0, ldx % 4 == 0 and the pointers are
 * 16-byte aligned, element loads otherwise).  means and prec (the precisions 1 / covariance; a spherical value repeated over
 * d) are dense f32 [K, D]; logc is fp64 [K], c_k = log w_k + sum_d log prec_kd / 2 - D log(2 pi) / 2.  Limits of every
 * entry: N, D, K >= 1 (else VSOM_EINVAL), K <= 1024 (else VSOM_EUNSUPPORTED), ldx >= D, ldr >= K (else VSOM_EINVAL).
 * Scratch is a TYPED array of doubles with an element count, sized by the host-only query vsom_gmm_parts(N, D, K, which)
 * (0 for a non-positive size or K > 1024); a count below the query or a null array is VSOM_EWORKSPACE before any launch.
 * No floating-point atomics; every sum has one fixed order: all outputs are bitwise reproducible. */
#define VSOM_GMM_ESTEP 0
#define VSOM_GMM_MSTEP 1 /* vsom_gmm_mstep and vsom_gmm_params: one array, handed from the first to the second */
#define VSOM_GMM_SET 2
long vsom_gmm_parts(long N, int D, int K, int which);
/* Rows of one M-step slab (the last may be shorter): the split is a function of the shape alone. */
long vsom_gmm_slab_rows(long N, int D, int K);
/* vsom_gmm_estep: the DIRECT form.  m_ik = sum_d (x_id - mu_kd)^2 prec_kd with f32 terms; the terms of a 4-column piece
 * (one column in the element path) are added in f32, the pieces of a lane in fp64 in column order, the 64 lanes by an
 * fp64 butterfly.  log p_ik = c_k - m_ik / 2 (fp64); log_prob_norm[i] (fp64 [N]) = the max-shifted fp64 log-sum-exp over
 * k; resp[i][k] (f32, row stride ldr; NULLABLE) = exp(log p_ik - log_prob_norm_i) rounded once; labels[i] (int64,
 * NULLABLE) = the first argmax of log p_ik, ties to the lowest k.  A row whose log_prob_norm is not finite (a NaN or an
 * infinity in X) is REFUSED: counted, its log_prob_norm and resp written as NaN, its label as -1.  part[g] / part[G + g]
 * receive workgroup g's sum of log_prob_norm over its accepted rows (wave by wave, rows ascending) and its refused rows;
 * estat (fp64 [2]) = their sums in g order.  The rest of part stages log p.  part: vsom_gmm_parts(.., VSOM_GMM_ESTEP). */
int vsom_gmm_estep(const float* X, long ldx, long N, int D, const float* means, const float* prec, const double* logc, int K,
                   float* resp, long ldr, double* log_prob_norm, int64_t* labels, double* estat, double* part, long n_part,
                   vsom_stream_t stream);
/* vsom_gmm_mstep: the partial sums of the M-step SHIFTED at means_old (f32 [K, D]: the previous means; the column means
 * repeated for the first M-step of a fit), per slab of vsom_gmm_slab_rows rows: nk_k = sum_i r_ik, S1_kd = sum_i r_ik e,
 * S2_kd = sum_i r_ik e^2 with e = x_id - means_old_kd, everything in fp64 (e and r e are exact), rows ascending. */
int vsom_gmm_mstep(const float* X, long ldx, long N, int D, const float* resp, long ldr, const float* means_old, int K,
                   double* part, long n_part, vsom_stream_t stream);
/* vsom_gmm_params: from the array vsom_gmm_mstep filled (it is also this entry's scratch), slabs added in slab order in
 * fp64: nk_k += 10 eps(fp64); a = S1 / nk; means (f32 [K, D], not means_old) = means_old + a; cov = S2 / nk - a^2 +
 * reg_covar (fp64 [K, D]; spherical != 0: fp64 [K], the mean over d in ascending d); prec = 1 / cov (f32 [K, D]);
 * weights (fp64 [K]) = nk / n_norm, or nk / sum_k nk (ascending k) when n_norm == 0; logc as above.  record (fp64 [8]):
 * [0] estat[0] / N, the lower bound of the E-step that made resp (NaN when estat is NULL), [1] the smallest nk, [2] the
 * smallest covariance, [3] the covariances that are <= 0 or not finite, [4] estat[1], the refused rows, [5] the weights'
 * divisor, [6..7] zero.  A component without responsibility keeps its mean (a = 0) and gets cov = reg_covar. */
int vsom_gmm_params(double* part, long n_part, long N, int D, int K, const float* means_old, double reg_covar, int spherical,
                    long n_norm, const double* estat, float* means, double* cov, float* prec, double* weights, double* logc,
                    double* record, vsom_stream_t stream);
/* vsom_gmm_set_params: prec, logc and record[2..3] from GIVEN weights (fp64 [K]) and covariances (fp64 [K, D] or, spherical,
 * [K]): what the E-step needs after an initialisation override, a warm start or a fit.  part: vsom_gmm_parts(1, D, K,
 * VSOM_GMM_SET) doubles. */
int vsom_gmm_set_params(const double* weights, const double* cov, int D, int K, int spherical, float* prec, double* logc,
                        double* record, double* part, long n_part, vsom_stream_t stream);

/* ------------------------------------------------------------------ small utilities */
int vsom_fill(float* p, long n, float value, vsom_stream_t stream);
/* out[0] = ca * a[0] + cb * b[0]: the step's total loss from its two device-side sums (vit_som.py:93,98); `counter`
   (nullable, one int64 on the device) is incremented by 1 in the same launch: `self.iteration += 1` (vit_som.py:104) */
int vsom_lincomb2(float* out, const float* a, float ca, const float* b, float cb, int64_t* counter, vsom_stream_t stream);
/* The step's loss terms in one launch (vit_som.py:93-102): parts[0] = total = main_scale * main_sum[0] + som_coef * som_sum[0]
   (som_coef = gamma_t / (B K): bitwise vsom_lincomb2's result), parts[1] = main_scale * main_sum[0] (reconstruction or
   cross-entropy term), parts[2] = som_scale * som_sum[0] (the SOM term before gamma); `counter` as in vsom_lincomb2. */
int vsom_loss_parts(float* parts, const float* main_sum, float main_scale, const float* som_sum, float som_coef,
                    float som_scale, int64_t* counter, vsom_stream_t stream);
/* out[i] = factor * (*scale_dev) * a[i] * b[i]  (b, scale_dev nullable -> 1): the elementwise products autograd needs
   for mean(weights * distances) (som_layer.py:137-142) with the upstream gradient as a device scalar */
int vsom_scaled_mul(float* out, const float* a, const float* b, long n, const float* scale_dev, float factor,
                    vsom_stream_t stream);
/* p[i] *= *scale_dev (a device scalar: no host sync) -- the incoming gradient of loss.backward(), applied to the
   loss-side gradient seeds before the backward kernels run (torch autograd's role at vit_som.py:80-105) */
int vsom_scale_by(float* p, long n, const float* scale_dev, vsom_stream_t stream);
/* out[j] = sum_s slabs[s*stride + j], j in [0,n) -- fixed summation order */
int vsom_reduce_slabs(const float* slabs, long stride, int nslabs, float* out, long n,
                      vsom_stream_t stream);

/* ------------------------------------------------------------------ agglomerative clustering (agglomerative.hip)
 * The two parts of sklearn.cluster.AgglomerativeClustering / scipy.cluster.hierarchy.linkage that cost time;
 * vit_som_amd/agglomerative.py drives them and cuts the tree, DESIGN.md section 4 has the algorithm; no counterpart in the
 * reference.  Limits of every entry: 1 <= N <= 16 384 (more: VSOM_EUNSUPPORTED with the bound in the message; the fp64
 * matrix is then 2 GiB).  No floating-point atomics, no cooperative launch, no loop that waits for another workgroup: all
 * outputs are bitwise reproducible.
 *
 * The workspace, vsom_agglo_workspace_bytes(N, connectivity) bytes (0 for N outside the limits), 8-byte aligned, holds at
 * byte 0 the fp64 [N, N] matrix (dense, row stride N), at byte (8 N^2 rounded up to 256) the [N, N] byte adjacency when
 * connectivity != 0, then the slots' state.  The caller fills the matrix (vsom_agglo_distances with out = the workspace,
 * ldo = N, or a matrix of its own) and the adjacency (symmetric, 0 / 1) before vsom_agglo_merge, which overwrites both. */
#define VSOM_AGGLO_EUCLIDEAN 0
#define VSOM_AGGLO_MANHATTAN 1
#define VSOM_AGGLO_COSINE 2
#define VSOM_AGGLO_WARD 0
#define VSOM_AGGLO_AVERAGE 1
#define VSOM_AGGLO_COMPLETE 2
#define VSOM_AGGLO_SINGLE 3
long vsom_agglo_workspace_bytes(long N, int connectivity);
/* vsom_agglo_distances: out[i, j] (fp64, row stride ldo >= N) for all i, j in the DIRECT form, every difference, product
 * and sum in fp64 on the f32 values of X [N, D] (row stride ldx; 16-byte loads when D % 4 == 0, ldx % 4 == 0 and X is
 * 16-byte aligned, element loads otherwise), columns ascending: euclidean sum_d (x - y)^2 (squared != 0) or its
 * correctly rounded square root; manhattan sum_d |x - y|; cosine max(0, 1 - x.y / sqrt(|x|^2 |y|^2)).  out[i, j] and
 * out[j, i] are the same bits, the diagonal is 0, identical rows are at exactly 0.  status (int32 [2], cleared here):
 * [0] the values of X that are NaN or infinite, [1] the rows of zero length (cosine: their distances are written as 1). */
int vsom_agglo_distances(const float* X, long ldx, long N, int D, int metric, int squared, double* out, long ldo, int* status,
                         vsom_stream_t stream);
/* vsom_agglo_merge: the generic greedy algorithm with a nearest-neighbour array on the workspace's matrix (SQUARED
 * euclidean distances for VSOM_AGGLO_WARD), N >= 2 (else VSOM_EINVAL).  Step s = 0 .. N - 2 merges the pair of active,
 * adjacent slots (a < b) that is least under the total order (distance, a, b); children[2 s], children[2 s + 1] (int32)
 * are the two clusters' ids in scipy's numbering (rows 0 .. N - 1, the cluster of step s is N + s), the smaller first;
 * distances[s] (fp64) is the pair's distance (its square root for Ward).  The merged cluster takes slot b; row and column
 * b follow the Lance-Williams update in fp64 without contraction; with connectivity != 0 the adjacency rows are OR-ed and
 * only adjacent clusters merge, at the FULL linkage distance over all their members.  3 (N - 1) + 2 launches are enqueued;
 * nothing is read back.  A step that finds no adjacent pair writes children -1, -1 and a NaN distance.  status (int32
 * [4]): [0] such steps (the graph's components less one), [1] slots other than b whose nearest neighbour was searched
 * again, [2] steps with such a slot, [3] zero.  ws too small or NULL: VSOM_EWORKSPACE; not 8-byte aligned: VSOM_EALIGN. */
int vsom_agglo_merge(void* ws, long ws_size, long N, int linkage, int connectivity, int* children, double* distances, int* status,
                     vsom_stream_t stream);

/* DBSCAN (Ester et al. 1996; sklearn.cluster.DBSCAN; vit_som_amd/dbscan.py; no counterpart in the reference): the
 * eps-neighbourhood graph as a bit matrix, the connected components of its core rows, sklearn's labels.  No entry takes a
 * caller-sized scratch buffer: every buffer is a typed output whose shape follows from N, and each needs only the natural
 * alignment of its type (hipMalloc and torch give more).  2 <= N <= 131 072 (2 GiB of bits; more: VSOM_EUNSUPPORTED).
 * No floating-point atomics, every sum in one fixed order: two runs are bitwise equal.
 *
 * The bit contract of adj (uint64 [N, W], W = ceil(N / 64), dense):
 *   bit (j & 63) of adj[i][j >> 6] is set iff rows i and j have a distance and it is <= eps;
 *   the diagonal is set (a row is in its own neighbourhood, as in sklearn);
 *   bits of columns >= N are clear;
 *   a bad row (the contract of vsom_knn_query: a NaN, an infinity, a squared norm that overflows fp32 -- euclidean: a
 *     squared distance to itself that does) has no bit set anywhere, in its row or its column;
 *   the matrix is symmetric bit for bit.
 * Every word is written exactly once (no need to clear adj), by a plain store: the result does not depend on the chunking.
 *
 * vsom_dbscan_neighbours: the contraction of vsom_knn_ranks with a thresholding epilogue.  The test is (double)d <= eps
 * with d bit for bit the fp32 distance of vsom_umap_knn between rows i and j of X [N, D] (row stride ldx >= D >= 1;
 * VSOM_DIST_EUCLIDEAN, with the root, or VSOM_DIST_COSINE; another metric: VSOM_EUNSUPPORTED) and eps >= 0 the caller's
 * double.  Rows are loaded 16 bytes per lane when D % 4 == 0, ldx % 4 == 0 and X is 16-byte aligned (the decision of
 * vsom_knn_ranks: operands of 4 GB or more take the element-wise loads), element-wise otherwise: the words are the same
 * bits either way.  Writes sq f32 [N] (the squared norms in the contraction's order), adj, count int32 [N] (the set bits
 * of row i, its own among them) and status int64 [2]: [0] the bad rows, [1] the set bits of the whole matrix.
 * vsom_dbscan_threshold: the same contract from a precomputed matrix M [N, N], float32 (is_f64 == 0) or float64, row
 * stride ldm >= N in elements: the test is (double)M[i][j] <= eps.  A NaN entry clears its bit; the diagonal is set
 * whatever it holds; the matrix is as symmetric as M is.  status[0] is the number of NaN entries (an integer atomic add),
 * status[1] the set bits. */
int vsom_dbscan_neighbours(const float* X, long ldx, long N, int D, int metric, double eps, float* sq, uint64_t* adj,
                           int32_t* count, int64_t* status, vsom_stream_t stream);
int vsom_dbscan_threshold(const void* M, long ldm, long N, int is_f64, double eps, uint64_t* adj, int32_t* count, int64_t* status,
                          vsom_stream_t stream);
/* The components of the core rows: int32 throughout, atomicMin the only atomic, no grid-wide barrier, no spin-wait.
 * vsom_dbscan_init: core[i] (uint8 [N]) = count[i] >= min_samples (>= 1); root[i] (int32 [N]) = i for a core row, -1
 * otherwise.
 * vsom_dbscan_round: clears changed (int32 [1]), then enqueues `rounds` (1 .. 1024) pairs of a hook step -- one wave per
 * core row: the least root[j] over the set bits j of its row with core[j], atomicMin-ed into root[i] and into
 * root[root[i]]; changed is raised when anything moved -- and a pointer-jumping step (roots only ever point to
 * smaller-or-equal indices, so the chase ends).  The caller repeats the call until changed stays 0.  The fixed point is
 * unique, every core row's root the smallest core row of its component, so the result does not depend on the races.
 * vsom_dbscan_finish, at the fixed point: a cluster's number is the rank of its root among the roots, ascending (sklearn's
 * numbering: it visits the rows in index order); a core row gets its root's number; a row that is not core gets the least
 * number among its core neighbours (sklearn expands the clusters in label order, so the first to reach a border point
 * has the smallest label), -1 without one.  Writes labels int64 [N] and record int32 [4]: clusters, core rows, border
 * rows, noise rows; core is the array vsom_dbscan_init wrote. */
int vsom_dbscan_init(const int32_t* count, long N, int min_samples, uint8_t* core, int32_t* root, vsom_stream_t stream);
int vsom_dbscan_round(const uint64_t* adj, long N, const uint8_t* core, int32_t* root, int rounds, int32_t* changed,
                      vsom_stream_t stream);
int vsom_dbscan_finish(const uint64_t* adj, long N, const uint8_t* core, const int32_t* root, int64_t* labels, int32_t* record,
                       vsom_stream_t stream);

/* HDBSCAN (Campello, Moulavi, Sander 2013; sklearn.cluster.HDBSCAN; vit_som_amd/hdbscan.py; no counterpart in the
 * reference): the minimum spanning tree of the mutual-reachability graph d_mr(i, j) = max(core[i], core[j], d(i, j)) by
 * Boruvka rounds, one contraction per round, the graph never held.  Undirected edges are ordered by (w, lo, hi), w the fp32
 * value of d_mr and lo < hi the rows: the order is strict, the tree unique, and Kruskal under the same order gives the same
 * N - 1 edges.  No entry takes a caller-sized scratch buffer: every buffer is typed and sized by N, at the natural
 * alignment of its type.  2 <= N <= 131 072 (more: VSOM_EUNSUPPORTED).  Integer atomics only, no grid-wide barrier, no
 * spin-wait, every device loop bounded by N: the edge list is bitwise reproducible.
 *
 * record (int32 [4]): [0] components left, [1] edges so far, [2] bad rows (matrix: bad entries), [3] rounds merged.
 * vsom_hdbscan_init: comp[i] (int32 [N]) = i; edges (int32 [N, 3]) = -1; record = (N, 0, 0, 0).
 * vsom_hdbscan_nearest: best[i] (uint64 [N], written in full) = the least (w, j) over the rows j with comp[j] != comp[i],
 * packed (fp32 bits of w) << 32 | j, all-ones without one.  d is bit for bit the fp32 distance of vsom_umap_knn between
 * rows of X [N, D] (row stride ldx >= D >= 1; VSOM_DIST_EUCLIDEAN, with the root, or VSOM_DIST_COSINE; another metric:
 * VSOM_EUNSUPPORTED); core (f32 [N]) the caller's core distances.  Rows are loaded 16 bytes per lane under the decision of
 * vsom_knn_ranks (operands of 4 GB or more take the element-wise loads), element-wise otherwise: the same bits.  Writes sq
 * f32 [N] (the squared norms) and record[2]: the rows with a NaN, an infinity, an overflowing norm or a core distance that
 * is not finite; such a row offers and receives nothing.
 * vsom_hdbscan_nearest_matrix: the same from a precomputed matrix M [N, N], float32 (is_f64 == 0) or float64, row stride
 * ldm >= N in elements: w = max(core[i], core[j], (float)M[i][j]), the fp32 rounding of the maximum.  An entry off the
 * diagonal that is not finite as fp32 offers nothing and is counted in record[2].
 * vsom_hdbscan_merge: per component the least of its rows' candidates under (w, lo, hi) (two integer atomicMin passes);
 * every component with one hooks onto the component at the other end -- of a mutual pair only the larger label -- and
 * writes (lo, hi, fp32 bits of w) to edges[label]; the hooks are chased to their roots and comp is relabelled; record[0],
 * [1] and [3] are updated.  A label is a row of its component; one that hooks is never a label again, so every slot of
 * edges is written at most once and only the last root's stays -1.  work: int64 [2 N], overwritten.  The caller repeats
 * nearest + merge until record[0] == 1: at most ceil(log2 N) rounds, since every round at least halves the components. */
int vsom_hdbscan_init(long N, int32_t* comp, int32_t* edges, int32_t* record, vsom_stream_t stream);
int vsom_hdbscan_nearest(const float* X, long ldx, long N, int D, int metric, const float* core, const int32_t* comp, float* sq,
                         uint64_t* best, int32_t* record, vsom_stream_t stream);
int vsom_hdbscan_nearest_matrix(const void* M, long ldm, long N, int is_f64, const float* core, const int32_t* comp, uint64_t* best,
                                int32_t* record, vsom_stream_t stream);
int vsom_hdbscan_merge(const uint64_t* best, long N, int32_t* comp, int32_t* edges, int64_t* work, int32_t* record,
                       vsom_stream_t stream);

/* Spectral embedding (Belkin and Niyogi 2003; sklearn.manifold.SpectralEmbedding; vit_som_amd/spectral.py; no counterpart
 * in the reference): the device side of a Chebyshev-filtered subspace iteration (Zhou and Saad 2007) on
 * M = D^-1/2 A D^-1/2.  A is a symmetric affinity in CSR -- int64 indptr [N + 1] / indices [nnz], fp64 data [nnz], the
 * convention of vsom_tsne_step -- whose diagonal entries are ignored; d are its row sums, s = d^-1/2.  Everything is fp64.
 * A block is row-major [N, l] with a row stride in elements, 1 <= l <= 32, 1 <= N <= 131 072 (more: VSOM_EUNSUPPORTED).
 * Every pointer needs only the natural alignment of its type; no entry has a 16-byte path.  No floating-point atomics, no
 * grid-wide barrier, no spin-wait: every sum has one order fixed by the operands, two runs are bitwise equal.
 *
 * The order of a row's sum: its entries are cut into chunks of 512 in CSR order; a chunk is one fma chain from 0, the
 * chunks' sums are added in chunk order.  A row of at most 512 entries is one chain.
 *
 * vsom_spectral_degrees: d[i] = the sum of row i without its diagonal entry, one chain in CSR order; s[i] = 1 / sqrt(d[i]),
 * 0 for a row without weight.  heavy (int32 [N]) receives the rows of more than 512 entries, in no particular order.
 * status (int64 [5], cleared here): [0] rows with d = 0, [1] indices outside [0, N), [2] weights that are negative or not
 * finite, [3] rows whose indptr pair is not 0 <= indptr[i] <= indptr[i + 1] <= nnz (read as empty), [4] the length of
 * heavy.  Entries counted in [1] or [2] are left out of the sums.  The caller refuses the matrix when [1..3] are not 0.
 * vsom_spectral_spmm: Yout = alpha (M Y1 - c Y1) - beta Y0, Y0 may be NULL; all blocks share ld.  Element (i, t) is
 * s_i * sum_j (a_ij s_j) Y1[j, t] in the order above, j == i and an index outside [0, N) skipped, then
 * alpha * fma(-c, Y1[i, t], .) and fma(-beta, Y0[i, t], .).  With heavy == NULL one group of lanes walks each row whatever
 * its length; with the list of vsom_spectral_degrees (all its n_heavy rows) each listed row gets a workgroup of its own:
 * the same bits.  Yout overlapping Y1 or Y0: VSOM_EINVAL.
 * vsom_spectral_ws_size: bytes of the workspace of vsom_spectral_gram and vsom_spectral_residual; 0 outside the limits.
 * The rows are cut into at most `slabs` (1 .. 1024) slabs of a multiple of 64 rows; a slab's sum is one chain over its rows
 * (residual: eight interleaved chains added in order), the slabs are added in slab order.  The result depends on N, l
 * and slabs alone.  ws NULL or short: VSOM_EWORKSPACE; not 8-byte aligned: VSOM_EALIGN.
 * vsom_spectral_gram: G = V^T V and, with W and H, H = V^T W; G and H fp64 [l, l] dense.
 * vsom_spectral_rotate: Vout [N, l_out] = V [N, l] T, T fp64 [l, l_out] dense on the device, the chain over l in index
 * order.  Vout overlapping V: VSOM_EINVAL.
 * vsom_spectral_residual: out[j] = sum_i (W[i, j] - theta[j] V[i, j])^2, from the differences themselves; theta, out fp64 [l].
 * vsom_spectral_embed: E[i, j] (f32, row stride lde) = sign[j] * (s[i] * V[i, first + j]), one rounding; sign[j] (fp64
 * [n_out], written) makes the entry of largest |s_i V_ij| positive, the smaller row on a tie (numpy's argmax, as in
 * sklearn's _deterministic_vector_sign_flip). */
int vsom_spectral_degrees(const int64_t* indptr, const int64_t* indices, const double* data, long N, long nnz, double* d, double* s,
                          int32_t* heavy, int64_t* status, vsom_stream_t stream);
int vsom_spectral_spmm(const int64_t* indptr, const int64_t* indices, const double* data, const double* s, long N, long nnz,
                       const int32_t* heavy, int n_heavy, const double* Y1, const double* Y0, double* Yout, long ld, int l,
                       double alpha, double c, double beta, vsom_stream_t stream);
long vsom_spectral_ws_size(long N, int l, int slabs);
int vsom_spectral_gram(const double* V, const double* W, long ld, long N, int l, int slabs, double* G, double* H, void* ws, long ws_size,
                       vsom_stream_t stream);
int vsom_spectral_rotate(const double* V, long ldv, long N, int l, const double* T, int l_out, double* Vout, long ldo,
                         vsom_stream_t stream);
int vsom_spectral_residual(const double* V, const double* W, long ld, long N, int l, const double* theta, int slabs, double* out,
                           void* ws, long ws_size, vsom_stream_t stream);
int vsom_spectral_embed(const double* V, long ldv, const double* s, long N, int first, int n_out, float* E, long lde, double* sign,
                        vsom_stream_t stream);

/* Attention rollout (Abnar and Zuidema 2020, head fusion as in the vit-explain recipe; vit_som_amd/attention_rollout.py; no
 * counterpart in the reference): one link of the vector-matrix chain that folds a stack of attention layers into one map
 * per image.  qkv is a block's saved [B N, 3 H hd] buffer, columns ordered [3][H][hd] as vsom_attention_probs reads it;
 * v_in, v_out are f32 [B, N] dense.  No N x N matrix is formed anywhere.
 *
 *   P_h[i, j] = softmax_j(q_i . k_j / sqrt(hd)), each row normalised by its own scores (the saved lse is not an argument)
 *   F[i, j]   = the mean (fusion 0), max (1) or min (2) over the heads of P_h[i, j]
 *   A[i, j]   = (alpha F[i, j] + (1 - alpha) [i == j]) / (alpha sum_j F[i, j] + (1 - alpha)),  0 < alpha <= 1
 *   v_out[b, j] = sum_i v_in[b, i] A_b[i, j]
 *
 * The minimum is taken of log P_h = (s - max) - log(sum) and exponentiated relative to the fused row's largest entry, the
 * row's scale returning as one factor (with alpha = 1 it cancels and is never formed): where saturated heads disagree
 * every min_h P_h of a row lies below the smallest float, and only their ratios are needed.
 * The order of every sum: a score is one fma chain over d ascending from 0, then scaled; a row's maximum and sum are a
 * lane's keys (j, j + 64, ...) in ascending order, then the wave's xor tree.  The column sum over i is cut into blocks of
 * 16 rows: inside a block each of four waves adds its four rows in ascending i (fp32 fma), the waves are added in wave
 * order, and the blocks of a sample are added in block order in fp64 and rounded once.  No atomics, no grid-wide barrier,
 * no spin-wait; two runs are bitwise equal and a sample's row depends neither on B nor on its place in the batch.
 *
 * Plain VALU, 4-byte accesses only: no pointer needs more than the alignment of a float, and no head dim is padded.
 * Limits: N <= 320 (five chunks of 64 keys) and (N (hd | 1) + 16 hd + 256 ceil(N / 64)) * 4 bytes of LDS <= 160 KiB -- every
 * project shape (N <= 257, hd <= 64) and any hd >= 1 that fits; otherwise VSOM_EUNSUPPORTED, the message naming N, hd and
 * the bytes.  A null pointer, a size <= 0, fusion outside {0, 1, 2}, alpha outside (0, 1], or v_out overlapping v_in:
 * VSOM_EINVAL.  ws NULL or short: VSOM_EWORKSPACE.  All of these before any launch.
 * vsom_attention_rollout_ws_size: bytes of the workspace (B ceil(N / 16) partial rows of N floats); 0 outside the limits. */
long vsom_attention_rollout_ws_size(int B, int N, int H, int hd);
int vsom_attention_rollout_step(const float* qkv, const float* v_in, float* v_out, int B, int N, int H, int hd, int fusion, float alpha,
                                void* ws, long ws_size, vsom_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* VITSOM_HIP_H */
