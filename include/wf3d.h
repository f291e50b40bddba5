/* wf3d.h — C ABI of libwf3d.so: the MI355X (gfx950) kernels behind the
 * PointNetEncoder -> VertexPredictor -> EdgePredictor forward/backward path.
 *
 * The reference (cansdev/wireframe-3d-prediction) has no FFI/operator layer: its
 * path is torch.nn modules calling ATen.  Each entry point
 * below therefore replaces the ATen op sequence of the cited reference lines;
 * the Python host (wireframe-3d-prediction_amd/wf3d/ops.py) binds them with
 * ctypes and the drop-in classes in wireframe-3d-prediction_amd/models/ call
 * them from torch.autograd.Function.  INTEGRATION.md shows the binding.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes only; every pointer is a DEVICE
 *     pointer borrowed for the call (no ownership taken, nothing allocated).
 *   - all tensors fp32, row-major, unless a name says otherwise
 *   - every call is asynchronous on `stream` (a hipStream_t passed as void*),
 *     never synchronises, never throws; returns WF3D_OK or a negative code and
 *     leaves a message for wf3d_last_error() (thread-local).
 *   - scratch comes from the caller: `ws` of at least the matching
 *     *_ws_bytes(...) bytes, 256-byte aligned.
 */
#ifndef WF3D_H
#define WF3D_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define WF3D_VERSION 105 /* 101: wf3d_gemm_t gained `x3`; 102: `lr_u`, `lr_v`, `lr_k`, `ld_lr_u`, `ld_lr_v` (all appended); 103: wf3d_set_option; 104: wf3d_edge_pair_ln_bwd, wf3d_edge_pair_fwd_ln accepts pre = NULL; 105: `vd` (coordinates per vertex, 1..8) in the edge-head entry points, wf3d_meter_update, wf3d_parse_table */

#define WF3D_OK 0
#define WF3D_ERR_ARG (-1)
#define WF3D_ERR_LAUNCH (-2)
#define WF3D_ERR_WS (-3)
#define WF3D_ERR_UNSUPPORTED (-4)

/* activations fused into prologues / elementwise kernels */
#define WF3D_ACT_NONE 0
#define WF3D_ACT_RELU 1 /* nn.ReLU   — PointNetEncoder.py:38, VertexPredictor.py:30 */
#define WF3D_ACT_GELU 2 /* nn.GELU (erf) — EdgePredictor.py:34,59,63,66 */

/* GEMM operand layouts (k = reduction index) */
#define WF3D_NT 0 /* C[M,N] = A[M,K] · B[N,K]^T  — nn.Linear forward  (aten::addmm) */
#define WF3D_NN 1 /* C[M,N] = A[M,K] · B[K,N]    — Linear dgrad  dX = dY·W           */
#define WF3D_TN 2 /* C[M,N] = A[K,M]^T · B[K,N]  — Linear wgrad  dW = dY^T·X         */

int wf3d_version(void);
const char* wf3d_last_error(void);

/* Process-wide run-time switches (everything else is per call).
 *   "tn_rounds" (1..8, default 1): workgroups per CU that the large weight-gradient launches of
 *       wf3d_gemm_split_tn are cut into.  1 is fastest on an idle chip; with a collective's kernels holding CUs beside
 *       the backward pass (data parallel) a launch of one workgroup per CU waits a whole extra
 *       round for its last workgroup (+67 %), 2 / 4 rounds lose 15 % / 0 % there and cost 2.5 % / 4 % otherwise.
 *   "gemm_cus" (0 = one workgroup per CU, the default; or 8..1024, rounded down to a multiple of 8): workgroups the
 *       persistent kernel of wf3d_gemm_split is launched with.  Its tiles are claimed, so fewer workgroups only leave
 *       CUs to whatever else the caller runs beside it (224 of 256 CUs: +9 % time; scripts/bench_overlap.py).
 *   "split_kernel" (0, 1, 3 or 6; for tests and diagnostics): 0 = automatic kernel choice, the default; 1 = the
 *       register-staged kernel for every wf3d_gemm_split / wf3d_gemm_bf16 call; 3 = 256x128 tiles for every split call
 *       (the three-stage LDS-DMA kernel forward / dgrad, the 256x128 kernel for wf3d_gemm_split_tn); 6 = the 256x256
 *       forward / dgrad kernel on every shape (wgrad keeps its automatic choice).  The workspace queries follow it, so
 *       a workspace sized under one value may be too small under another (the launch then does not split K).
 *   "attn_tiled" (0, 1 or 2): which calls of wf3d_attn_fwd / wf3d_attn_bwd run on the key-tiled MFMA kernels.
 *       1 = automatic, the default: head_dim 64 with vmax > 256 (smaller ones keep the kernels that hold a whole
 *       sample in LDS), and every head_dim in 68..128 at every vmax; 0 = never (head_dim 64 with vmax > 256 and every
 *       head_dim in 68..128 then run on the VALU kernels, which refuse a head_dim above 64 beyond their LDS limit; for
 *       A/B timing and tests); 2 = every call with a head_dim in 64..128 whatever vmax (for tests and diagnostics).
 *       Head widths up to 60 and above 128 run on the VALU kernels under every value.  wf3d_attn_kernel reports the
 *       outcome.
 * Returns WF3D_OK, or WF3D_ERR_ARG for an unknown name or a value out of range. */
int wf3d_set_option(const char* name, int value);

/* ------------------------------------------------------------------------
 * wf3d_gemm — fp32 MFMA (v_mfma_f32_32x32x2_f32) GEMM with a fused
 * LayerNorm-affine + activation (+dropout) PROLOGUE on the activation operand
 * and a bias / residual / accumulate EPILOGUE.
 *
 * Replaces, per reference Linear: aten::addmm (+ the native_layer_norm apply,
 * relu_/gelu and dropout that precede it), e.g. PointNetEncoder.py:35-45,94;
 * VertexPredictor.py:27-61,105-117; EdgePredictor.py:31-38,56-68,106,137;
 * and in backward the two mm's autograd derives per Linear.
 *
 * Prologue (applied while the operand tile is staged into LDS), on operand A
 * for WF3D_NT and on operand B for WF3D_TN, over that operand's own [rows, cols]
 * global shape:   v' = drop( act( (v - mu[row]) * rs[row] * gamma[col] + beta[col] ) )
 * pro_mu == NULL skips the LayerNorm part (v' = drop(act(v))).
 * ------------------------------------------------------------------------ */
typedef struct wf3d_gemm_t {
    const float* A;
    const float* B;
    float* C;
    const float* bias;   /* [N] or NULL                                         */
    const float* addend; /* [M, ld_addend] added in the epilogue, or NULL       */
    int M, N, K;
    int lda, ldb, ldc, ld_addend;
    int layout;          /* WF3D_NT / WF3D_NN / WF3D_TN                        */
    int pro_act;         /* WF3D_ACT_*; prologue enabled iff pro_enable != 0    */
    int pro_enable;
    const float* pro_mu;    /* [rows] or NULL */
    const float* pro_rs;    /* [rows]         */
    const float* pro_gamma; /* [cols] or NULL (NULL with pro_mu == NULL)        */
    const float* pro_beta;  /* [cols]         */
    float drop_p;           /* 0 = no dropout; else keep-prob 1-p, scaled 1/(1-p) */
    uint32_t drop_seed;
    int accumulate;      /* C += result instead of C = result                   */
    void* ws;            /* split-K slabs, wf3d_gemm_ws_bytes() bytes, or NULL  */
    size_t ws_bytes;
    int x3;              /* 0: exact fp32 MFMA.  1: bf16x3 arithmetic — the fp32 operands (after the prologue) are
                            split into bf16 (hi, lo) while they are staged into LDS and multiplied as
                            hi*hi + hi*lo + lo*hi on v_mfma_f32_32x32x16_bf16 (fp32 accumulate; relative error
                            ~2^-16 per product).  Ignored for M <= 64 (32-row tile).                       */
    const float* lr_u;   /* epilogue low-rank term  C += U[M, lr_k] . V[N, lr_k]^T  (exact fp32), lr_k = 0..4, 0 = none:  */
    const float* lr_v;   /* the coordinate columns of the first edge Linear — Pa = F.Wa^T + c.Wc^T, EdgePredictor.py:     */
    int lr_k;            /* 130-137 — ride on the GEMM that already writes Pa instead of a K = 3 GEMM with accumulate      */
    int ld_lr_u, ld_lr_v;
} wf3d_gemm_t;

size_t wf3d_gemm_ws_bytes(int M, int N, int K, int layout);
int wf3d_gemm(const wf3d_gemm_t* desc, void* stream);

/* ------------------------------------------------------------------------
 * bf16x3 split-precision path for the large Linear layers (same results as the
 * fp32 path to ~1e-5, 3 bf16 MFMAs per product instead of one fp32 MFMA at 1/16
 * of the bf16 rate).  Operands are in the "sx8" format: a logical fp32 [R, C]
 * matrix (C % 8 == 0) with the same bytes/pitch as fp32, each 32-byte group of
 * 8 consecutive columns holding [8 x bf16 high | 8 x bf16 low], v ~= hi + lo.
 * Every producer writes hi = bf16_rne(v), lo = bf16_rne(v - hi), so that
 * |v - hi - lo| <= 2^-17 |v| (finite v whose hi and lo are normal bf16 numbers;
 * tests/sx8_model.py states the split on integer bits).  The pair is NOT a
 * function of the sum hi + lo: where lo was rounded up onto half an ulp of an odd
 * hi, splitting hi + lo again gives the even neighbour and the opposite low part.
 * An entry point that takes an sx8 input and hands it on moves the two planes.
 * ------------------------------------------------------------------------ */
/* C[M,N] (+)= A·B^T + bias, A = sx8[M,K], B = sx8[N,K] (nn.Linear forward with
 * B = W; its dgrad with A = dY, B = W^T in sx8).  The workspace is written by every call that is given one (split-K
 * slabs, or the persistent kernel's tile-claim counters), so launches that may run concurrently must not share it. */
size_t wf3d_gemm_split_ws_bytes(int M, int N, int K);
int wf3d_gemm_split(const void* A_sx8, const void* B_sx8, float* C, const float* bias, int M, int N, int K,
                    int lda, int ldb, int ldc, int accumulate, void* ws, size_t ws_bytes, void* stream);
/* C[Mo,No] (+)= A^T·B with A = sx8[K,Mo], B = sx8[K,No]: the Linear wgrad dW = dY^T·X on the
 * operands exactly as backward/forward leave them (no transposed copies; fragments are gathered
 * with ds_read_b64_tr_b16).  Supported when wf3d_gemm_split_tn_ok() (Mo % 256, No % 128, K % 32). */
int wf3d_gemm_split_tn_ok(int Mo, int No, int K, int lda, int ldb);
size_t wf3d_gemm_split_tn_ws_bytes(int Mo, int No, int K);
int wf3d_gemm_split_tn(const void* A_sx8, const void* B_sx8, float* C, int Mo, int No, int K, int lda, int ldb,
                       int ldc, int accumulate, void* ws, size_t ws_bytes, void* stream);
/* bf16 arithmetic (opt-in precision mode "bf16"): the same two products, one bf16 MFMA per product on the
 * hi planes of the sx8 operands (hi = bf16 round-to-nearest of v; the lo planes are not read), fp32 accumulation.
 * Same signatures, argument checks, error codes, accepted shapes / layouts and kernel selection as
 * wf3d_gemm_split / wf3d_gemm_split_tn; the workspace is sized by wf3d_gemm_split_ws_bytes /
 * wf3d_gemm_split_tn_ws_bytes. */
int wf3d_gemm_bf16(const void* A_sx8, const void* B_sx8, float* C, const float* bias, int M, int N, int K,
                   int lda, int ldb, int ldc, int accumulate, void* ws, size_t ws_bytes, void* stream);
int wf3d_gemm_bf16_tn(const void* A_sx8, const void* B_sx8, float* C, int Mo, int No, int K, int lda, int ldb,
                      int ldc, int accumulate, void* ws, size_t ws_bytes, void* stream);
/* Which kernel a wf3d_gemm_split / wf3d_gemm_bf16 call (wf3d_gemm_split_tn / wf3d_gemm_bf16_tn: the _tn query) with
 * these arguments takes, under the options in force: the launch path decides through the same host function.  Nothing is
 * launched and nothing is written but route[0..7]: kernel form (WF3D_SPLIT_FORM_*), K ranges after the workspace fit, K
 * slices per range, 1 if the wgrad grid is the XCD-mapped 1-D one, combine kind (WF3D_SPLIT_COMBINE_*), tile rows,
 * tile columns, workgroups of the persistent kernel (0 for every other form).  C, bias and ws are looked at as
 * addresses only (alignment, NULL).  cus: the device's compute-unit count; 0 asks the current device, any other value
 * needs no device.  Returns WF3D_OK, or what the call itself returns for dimensions it refuses (and WF3D_ERR_ARG for an
 * empty output, which a call accepts and no kernel serves). */
#define WF3D_SPLIT_FORM_REGS 0    /* register-staged 128x128 (K % 32 != 0, or split_kernel 1) */
#define WF3D_SPLIT_FORM_DMA3 1    /* 256x128, three LDS stages */
#define WF3D_SPLIT_FORM_X16 2     /* 256x256 on the 16x16x32 MFMA, one workgroup per tile */
#define WF3D_SPLIT_FORM_X16P 3    /* its persistent, tile-claiming form */
#define WF3D_SPLIT_FORM_DMA3_TN 4 /* wgrad, 256x128 */
#define WF3D_SPLIT_FORM_X16_TN 5  /* wgrad, 256x256 */
#define WF3D_SPLIT_COMBINE_NONE 0
#define WF3D_SPLIT_COMBINE_NARROW 1 /* slab after slab */
#define WF3D_SPLIT_COMBINE_WIDE 2   /* 16 strided partial sums per output (more than 16 slabs, N % 4 == 0) */
int wf3d_gemm_split_route(int M, int N, int K, int lda, int ldb, int ldc, const void* C, const void* bias, int accumulate,
                          const void* ws, size_t ws_bytes, int cus, int* route);
int wf3d_gemm_split_tn_route(int Mo, int No, int K, int lda, int ldb, int ldc, int accumulate, const void* ws,
                             size_t ws_bytes, int* route);
/* out_sx8[r, c] = split(in[r*row_stride + c*col_stride])  (col_stride 1: convert;
 * row_stride 1: transpose-convert, used for W^T) */
int wf3d_split_rows(const float* in, long row_stride, long col_stride, int R, int C, void* out_sx8, void* stream);
/* the same for up to 8 matrices in one launch (host arrays of length njobs): a stage's weights, each as W and as W^T */
int wf3d_split_rows_multi(const float* const* in, const long* row_stride, const long* col_stride, const int* R, const int* C,
                          void* const* out_sx8, int njobs, void* stream);
/* out_sx8[C, R] = split(drop(act(LN-affine(in[R, C]))))^T — the wgrad operands (reduction
 * index = row index made contiguous): dW = dY^T·X becomes the NT-form
 * wf3d_gemm_split(dY^T_sx8, X^T_sx8).  mu/gamma NULL skip the respective part;
 * in_sx8 != 0: `in` is itself an sx8 matrix (no prologue), transposed plane-wise:
 * out's high and low planes are the input's, bit for bit (no second split). */
int wf3d_split_transpose(const float* in, int R, int C, int ld, const float* mu, const float* rs,
                         const float* gamma, const float* beta, int act, float drop_p, uint32_t drop_seed,
                         int in_sx8, void* out_sx8, void* stream);
/* LayerNorm statistics of z[R,D] AND h = drop(act(LN(z))) in sx8, one read of z:
 * the operand producer between two split GEMMs (replaces native_layer_norm +
 * relu_ of PointNetEncoder.py:36-38 in the split path). */
int wf3d_ln_prep(const float* z, int R, int D, const float* gamma, const float* beta, int act, float eps,
                 float drop_p, uint32_t drop_seed, float* mu, float* rs, void* h_sx8, void* stream);
/* First Linear of the per-point MLP (in_features K <= 8) fused with its LayerNorm / activation / split
 * (models/PointNetEncoder.py:35-45, layer 0): writes z = x·W^T + b [R, D] (kept for backward), (mu, rstd) and
 * h = act(LN(z)) in sx8 — one pass instead of a GEMM that writes z plus a normalisation pass that reads it back. */
int wf3d_first_layer_fwd(const float* x, int R, int K, int ldx, const float* W, int ldw, const float* bias, int D,
                         const float* gamma, const float* beta, int act, float eps, float* z, float* mu, float* rs,
                         void* h_sx8, void* stream);
/* The same with the train-mode dropout that follows the activation (PointNetEncoder.mlp[3], p > 0 in train() mode):
 * h = drop(act(LN(z))) — exact zeros where element (row, col) is dropped, the kept value times 1 / (1 - drop_p) in fp32
 * elsewhere, the keep bit that of every other mask kernel for (drop_seed, row, col) — while z, mu and rs are the bits
 * wf3d_first_layer_fwd writes.  drop_seed is a value, or an index into the calling thread's device seed words
 * (wf3d_set_dropout_seed_words); the live-row count is honoured as by wf3d_first_layer_fwd.  drop_p = 0 (or below 2^-32)
 * is wf3d_first_layer_fwd itself: the same launch, no seed is read. */
int wf3d_first_layer_fwd_drop(const float* x, int R, int K, int ldx, const float* W, int ldw, const float* bias, int D,
                              const float* gamma, const float* beta, int act, float eps, float drop_p, uint32_t drop_seed,
                              float* z, float* mu, float* rs, void* h_sx8, void* stream);
/* ... and its backward: LayerNorm/activation backward of layer 0 that also accumulates that layer's weight
 * gradient dW[D, K] = dz^T·x (K more weighted column sums) and never writes dz (the input takes no gradient).
 * dgamma, dbeta, dbias must be one contiguous [3][D] buffer. */
size_t wf3d_ln_act_bwd_first_ws_bytes(int R, int D);
int wf3d_ln_act_bwd_first(const float* dh, const float* z, const float* x, int R, int D, int K, int ldx,
                          const float* mu, const float* rs, const float* gamma, const float* beta, int act,
                          float* dgamma, float* dbeta, float* dbias, float* dW, void* ws, size_t ws_bytes, void* stream);
/* The same as the backward of wf3d_first_layer_fwd_drop: dh is multiplied by the mask of (drop_seed, row, col) and
 * 1 / (1 - drop_p) where the row enters, so dgamma, dbeta, dbias and dW are sums over the masked dh.  Workspace, buffers
 * and the live-row count as wf3d_ln_act_bwd_first, which is this call with drop_p = 0. */
int wf3d_ln_act_bwd_first_drop(const float* dh, const float* z, const float* x, int R, int D, int K, int ldx,
                               const float* mu, const float* rs, const float* gamma, const float* beta, int act,
                               float drop_p, uint32_t drop_seed, float* dgamma, float* dbeta, float* dbias, float* dW,
                               void* ws, size_t ws_bytes, void* stream);
/* LayerNorm / activation backward that also returns one weighted column sum of the dz it produces,
 * wsum[c] = sum_r dz[r, c] * wrow[r] — for the first edge layer (models/EdgePredictor.py:130-137) the gradient of the
 * weight column that multiplies the pair distance — instead of a second pass over dz.  dgamma, dbeta: one [2][D] buffer. */
size_t wf3d_ln_act_bwd_wsum_ws_bytes(int R, int D);
int wf3d_ln_act_bwd_wsum(const float* dh, const float* z, const float* wrow, int R, int D, const float* mu, const float* rs,
                         const float* gamma, const float* beta, int act, float drop_p, uint32_t drop_seed, float* dz,
                         void* dz_sx8, float* dgamma, float* dbeta, float* wsum, void* ws, size_t ws_bytes, void* stream);


/* ------------------------------------------------------------------------
 * LayerNorm pieces (nn.LayerNorm, eps 1e-5, biased variance — SURVEY App. A)
 * ------------------------------------------------------------------------ */
/* mu[r], rs[r] = mean, 1/sqrt(var+eps) of row r of z[R, D] (row stride ld).
 * Replaces the statistics half of aten::native_layer_norm. */
int wf3d_row_stats(const float* z, int R, int D, int ld, float eps, float* mu, float* rs, void* stream);

/* out[r,c] = drop(act(LN(z)))[r,c] + addend[r,c]  (materialising form, used
 * where the value has several consumers: VertexPredictor.py:110,114 residual
 * sums, EdgePredictor.py:106,114).  mu == NULL skips the LayerNorm. */
int wf3d_ln_act_apply(const float* z, int R, int D, const float* mu, const float* rs,
                      const float* gamma, const float* beta, int act, const float* addend,
                      float drop_p, uint32_t drop_seed, float* out, void* stream);

/* Backward of h = drop(act(LN(z))) given dh: writes dz (may alias dh) and the
 * column reductions dgamma[D], dbeta[D] (LayerNorm affine grads) and
 * dbias[D] = sum_r dz[r,:] (the preceding Linear's bias grad).  Any of the
 * three outputs may be NULL; dz_sx8 (optional) receives dz in the sx8 split format
 * for wf3d_gemm_split, and then dz itself may be NULL.  Replaces native_layer_norm_backward +
 * threshold_backward / gelu_backward + the bias sum. */
size_t wf3d_ln_act_bwd_ws_bytes(int R, int D);
int wf3d_ln_act_bwd(const float* dh, const float* z, int R, int D, const float* mu, const float* rs,
                    const float* gamma, const float* beta, int act, float drop_p, uint32_t drop_seed,
                    float* dz, void* dz_sx8, float* dgamma, float* dbeta, float* dbias, void* ws,
                    size_t ws_bytes, void* stream);

/* out[c] = sum_r act(x[r,c]) * (w ? w[r] : 1)   — bias grads of Linears with no LN
 * behind them, the distance-weight grad of the split edge layer, and the weight
 * grad of a 1-output Linear (edge_mlp.10: dW[c] = sum_r dlogit[r] * gelu(z[r,c])). */
size_t wf3d_colsum_ws_bytes(int R, int D);
int wf3d_colsum(const float* x, int R, int D, int ld, const float* w, int act, float* out, void* ws,
                size_t ws_bytes, void* stream);

/* One-output Linear on act(z) — the logits layer edge_mlp[9..10] (models/EdgePredictor.py:66-67) — as a row dot
 * product, D = 8 * 2^k <= 512:  out[r] = bias[0] + sum_c act(z[r,c]) * w[c].
 * Backward, fused with the activation backward below it: dz[r,c] = dlogit[r] * w[c] * act'(z[r,c]) (fp32 and / or
 * sx8), dw[c] = sum_r dlogit[r] * act(z[r,c]), dbias_z[c] = sum_r dz[r,c]; dw and dbias_z are one [2][D] buffer. */
int wf3d_rowdot_act_ok(int D);
int wf3d_rowdot_act(const float* z, int R, int D, const float* w, const float* bias, int act, float* out, void* stream);
size_t wf3d_rowdot_act_bwd_ws_bytes(int R, int D);
int wf3d_rowdot_act_bwd(const float* z, const float* dlogit, int R, int D, const float* w, int act, float* dz,
                        void* dz_sx8, float* dw, float* dbias_z, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------
 * "Skinny" Linear layers: M <= 32 rows (one per cloud of the batch) — the feature-fusion MLP
 * (models/PointNetEncoder.py:57-65,116) and the vertex head (models/VertexPredictor.py:94-117),
 * forward and backward.  Replaces, per nn.Linear: aten::addmm, the native_layer_norm / relu_ in
 * front of it and the residual add behind it; in backward the two mm's, native_layer_norm_backward,
 * threshold_backward and the bias sum.  Pure weight streaming (csrc/skinny.hip): LayerNorm
 * statistics travel as per-16-column (mean, M2) partials from the producing launch to the
 * consuming one, the LayerNorm backward's row sums as per-64-column partials, so neither pass
 * exists as a kernel.  Up to WF3D_SKINNY_MAX_PROBLEMS Linears per launch.
 * ------------------------------------------------------------------------ */
#define WF3D_SKINNY_MAX_ROWS 32
#define WF3D_SKINNY_MAX_PROBLEMS 4

/* Y[M,N] = x'·W^T + bias + out_addend,  x' = act(LayerNorm(X; gamma, beta)) + in_addend  (gamma NULL: x' = X + in_addend).
 * LayerNorm statistics of X: merged from in_part [in_nblk = K/16][M][2] (what the launch that wrote X left in its
 * stat_part) and, when mu_out != NULL, stored to mu_out/rs_out [M] for backward; or given as mu/rs [M]. */
typedef struct wf3d_skinny_fwd_t {
    const float* X; int ldx;
    const float* W; int ldw;            /* [N, K] (nn.Linear weight) */
    const float* bias;                  /* [N] or NULL */
    float* Y; int ldy;
    int N, K;
    const float* gamma; const float* beta; int act;      /* input prologue (WF3D_ACT_*) */
    const float* in_part; int in_nblk;  /* statistics partials of X, or NULL */
    const float* mu; const float* rs;   /* ... or final statistics */
    float* mu_out; float* rs_out;       /* [M] or NULL */
    const float* in_addend; int ld_in_addend;
    const float* out_addend; int ld_out_addend;
    float* stat_part;                   /* [N/16][M][2] (mean, M2) of Y per 16-column block, or NULL (needs N % 16 == 0) */
} wf3d_skinny_fwd_t;
int wf3d_skinny_ok(int M, int K);
int wf3d_skinny_fwd(const wf3d_skinny_fwd_t* probs, int nprob, int M, float eps, void* stream);

/* Backward of one Linear y = x'·W^T + b given the gradient of its output:
 *   plain form (z == NULL):  dz = dY
 *   LayerNorm form:          dY holds G = dh * act'(LN(z)) * gamma (wf3d_skinny_reduce), z/mu/rs this Linear's own
 *                            pre-LayerNorm output and statistics, rowpart [rowpart_nblk][M][2] the partial row sums of
 *                            (G, G*xhat):  dz = rs * (G - mean(G) - xhat * mean(G*xhat))
 * Outputs: dW[N,K] = dz^T·x' and db[N] = colsum(dz) (x' rebuilt from X with the forward's prologue; dW NULL skips
 * both), and slabs [ceil(N/nc)][M][K]: partial dgrad dX_s = dz[:, s*nc:(s+1)*nc]·W[s*nc:(s+1)*nc, :] (NULL skips). */
typedef struct wf3d_skinny_bwd_t {
    const float* dY; int lddy;
    const float* z; int ldz; const float* mu; const float* rs; const float* rowpart; int rowpart_nblk;
    const float* W; int ldw; int N, K;
    const float* X; int ldx;
    const float* xmu; const float* xrs; const float* xgamma; const float* xbeta; int xact;
    const float* xadd; int ldxadd;
    float* dW; int lddw; float* db;
    float* slabs; int nc;               /* nc: any even chunk height in 2..128 (a multiple of 4, with N % 4 == 0 and 16-byte
                                           aligned dY / z rows, loads dz 16 bytes per lane; every other case by element) */
} wf3d_skinny_bwd_t;
size_t wf3d_skinny_slab_floats(int M, int N, int K, int nc);
int wf3d_skinny_bwd(const wf3d_skinny_bwd_t* probs, int nprob, int M, void* stream);

/* v[M,K] = sum of up to three slab sets (fixed order: deterministic) + extra; optionally stored to dh.  With z != NULL
 * v is the gradient of h = act(LayerNorm(z)) and the elementwise half of that backward is applied in the same pass:
 * G = v*act'*gamma -> G[M,K], dgamma[K], dbeta[K], rowpart [ceil(K/64)][M][2] = per-block row sums of (G, G*xhat). */
typedef struct wf3d_skinny_red_t {
    const float* slabs[3]; int nslab[3];
    const float* extra; int ldextra;
    int K;
    float* dh; int lddh;
    const float* z; int ldz; const float* mu; const float* rs; const float* gamma; const float* beta; int act;
    float* G; int ldg; float* dgamma; float* dbeta; float* rowpart;
} wf3d_skinny_red_t;
int wf3d_skinny_reduce(const wf3d_skinny_red_t* prob, int M, void* stream);

/* ------------------------------------------------------------------------
 * Pools (PointNetEncoder.py:85-86,103-111 and VertexPredictor.py:86-88)
 * ------------------------------------------------------------------------ */
/* valid[m] = (sum_k |x[m,k]| > 1e-9) ? 1 : 0 */
int wf3d_point_valid(const float* x, int M, int in_dim, float* valid, void* stream);

/* One pass over point_features pf[B,N,C] producing all four reductions the two
 * heads need: masked max (0 where a cloud has no valid point) + its first-max
 * index, masked mean over max(count,1), unmasked mean, unmasked max + index,
 * and cnt[b] = max(#valid, 1). */
size_t wf3d_pool4_ws_bytes(int B, int N, int C);
/* The four pooled [B, C] outputs are written with row stride ldo (>= C), so that [max | avg] and [mean | max] can be
 * the two halves of the [B, 2C] vectors the fusion MLP / the vertex head consume (the reference's torch.cat,
 * PointNetEncoder.py:115, VertexPredictor.py:88); nvalid[b] (optional) = the unclamped number of valid points. */
int wf3d_pool4_fwd(const float* pf, const float* valid, int B, int N, int C, float* mmax, float* mavg,
                   float* umean, float* umax, int ldo, int32_t* arg_m, int32_t* arg_u, float* cnt, float* nvalid,
                   void* ws, size_t ws_bytes, void* stream);
/* dpf[b,n,c] = valid*dmavg/cnt + dumean/N + [n==arg_m]*dmmax + [n==arg_u]*dumax (+ dpf_direct);
 * the masked / unmasked cotangent pairs have row strides ldm / ldu (halves of [B, 2C] gradients). */
int wf3d_pool4_bwd(const float* valid, const float* cnt, const int32_t* arg_m, const int32_t* arg_u,
                   const float* dmmax, const float* dmavg, int ldm, const float* dumean, const float* dumax, int ldu,
                   const float* dpf_direct, int B, int N, int C, float* dpf, void* stream);
/* dbias[c] = sum over all B*N rows of the dpf above without dpf_direct — the bias gradient of the Linear that
 * produced point_features (encoder.mlp.16) — from the [B, C] cotangents alone. */
int wf3d_pool4_bwd_bias(const float* cnt, const float* nvalid, const int32_t* arg_m, const int32_t* arg_u,
                        const float* dmmax, const float* dmavg, int ldm, const float* dumean, const float* dumax, int ldu,
                        int B, int C, float* dbias, void* stream);
/* Same values written as the sx8 split operand of the output Linear's dgrad / wgrad GEMMs (C % 8 == 0):
 * saves the fp32 round trip through wf3d_split_rows. */
int wf3d_pool4_bwd_sx8(const float* valid, const float* cnt, const int32_t* arg_m, const int32_t* arg_u,
                       const float* dmmax, const float* dmavg, int ldm, const float* dumean, const float* dumax, int ldu,
                       const float* dpf_direct, int B, int N, int C, float* dpf_sx8, void* stream);

/* PACKED batches: the clouds of a batch concatenated along the point axis, pf[M_pad, C] with cloud b in rows
 * rows[b] .. rows[b+1]-1 (rows[0] = 0, rows[B] = M) and M_pad >= M; rows M .. M_pad-1 belong to no cloud.
 * The work is described by a chunk table built from the point counts (int32, device memory, 16-byte aligned; by the host,
 * or on the device in the capacity form below):
 *   chunks[4k .. 4k+3] = (cloud b, rows[b], r0, r1)   rows r0 .. r1-1, all of cloud b; a cloud's chunks are consecutive
 *                                                     and in row order: cchunk[b] .. cchunk[b+1]-1
 *   (-1, 0, M, M_pad)                                 the pad rows, the last entry when M_pad > M (backward only)
 * wf3d_pool4_seg_fwd is wf3d_pool4_fwd over those row ranges: one partial result per chunk (the first nchunk entries,
 * without the pad chunk), folded per cloud in chunk order by a second kernel, so the result does not depend on how the
 * chip schedules the chunks.  Arg-max indices are local to the cloud (0 <= n < N_b), the unmasked mean divides by N_b,
 * cnt / nvalid are per cloud as in the dense form.  Pad rows are never read. */
size_t wf3d_pool4_seg_ws_bytes(int nchunk, int C);
int wf3d_pool4_seg_fwd(const float* pf, const float* valid, const int32_t* rows, const int32_t* cchunk,
                       const int32_t* chunks, int B, int M, int nchunk, int C, float* mmax, float* mavg,
                       float* umean, float* umax, int ldo, int32_t* arg_m, int32_t* arg_u, float* cnt,
                       float* nvalid, void* ws, size_t ws_bytes, void* stream);
/* wf3d_pool4_bwd / wf3d_pool4_bwd_sx8 over the same table (nchunk counts the pad chunk here; chunk_rows = the longest
 * chunk): dpf[M_pad, C], its pad rows exact zeros; dpf_direct, when given, has at least M rows.  The bias column sum of
 * a packed batch is wf3d_pool4_bwd_bias itself: it reads the [B, C] cotangents alone and does not depend on the rows. */
int wf3d_pool4_seg_bwd(const float* valid, const float* cnt, const int32_t* arg_m, const int32_t* arg_u,
                       const float* dmmax, const float* dmavg, int ldm, const float* dumean, const float* dumax,
                       int ldu, const float* dpf_direct, const int32_t* rows, const int32_t* chunks, int B, int M,
                       int M_pad, int nchunk, int chunk_rows, int C, float* dpf, void* stream);
int wf3d_pool4_seg_bwd_sx8(const float* valid, const float* cnt, const int32_t* arg_m, const int32_t* arg_u,
                           const float* dmmax, const float* dmavg, int ldm, const float* dumean, const float* dumax,
                           int ldu, const float* dpf_direct, const int32_t* rows, const int32_t* chunks, int B, int M,
                           int M_pad, int nchunk, int chunk_rows, int C, float* dpf_sx8, void* stream);

/* PACKED batches, capacity form: the same tables for a fixed row capacity (a multiple of 256), so that every launch shape
 * depends on (B, capacity) alone and the point counts may stay in device memory.  chunk_rows = max(256, 64 *
 * ceil(ceil(capacity / 256) / 64)), M_pad = capacity, and the table always has nchunk_cap = ceil(capacity / chunk_rows)
 * + B + 1 entries (wf3d_packed_layout_dims), forward and backward alike:
 *   1. the clouds' chunks as above (pieces of at most chunk_rows rows, cloud by cloud);
 *   2. (-1, 0, r0, r1): the pad rows M .. capacity-1 in pieces of at most chunk_rows rows;
 *   3. (-1, 0, capacity, capacity): dead entries up to nchunk_cap.
 * The forward skips every entry of cloud -1; the backward writes exact zeros to the rows of one (none for a dead entry).
 * Call the pools with nchunk = nchunk_cap, M_pad = capacity and M = capacity (M is only checked on the host; the live total
 * is rows[B], in device memory); dpf_direct, when given, has capacity rows.  Results per live chunk do not depend on how
 * many pad or dead entries follow.
 * wf3d_packed_layout_build writes rows [B+1], cchunk [B+1], chunks [4 * nchunk_cap] (16-byte aligned) and *status from
 * counts [B] in device memory (int64; _i32: int32): one launch of one workgroup, plain stores, no host read, nothing but
 * (B, capacity) decides the launch.  It clamps instead of failing: a negative count is 0, a cloud that would pass
 * `capacity` ends there and the clouds after it get no rows.  *status bit 0: something was clamped for capacity; bit 1:
 * some cloud has no rows.  wf3d.ops.PackedLayout(counts, capacity) is the same table built on the host, integer for
 * integer.
 * A cloud of no rows (cchunk[b] == cchunk[b+1]) pools like the dense form's all-padded cloud where that is defined and to
 * zeros elsewhere: mmax = mavg = umean = umax = 0, arg_m = arg_u = -1, cnt = 1 (the clamp), nvalid = 0.  Its backward
 * writes no row, and wf3d_pool4_bwd_bias leaves its dumean / dumax out of the column sum (arg_u < 0). */
int wf3d_packed_layout_dims(int B, int capacity, int* chunk_rows, int* nchunk_cap);
int wf3d_packed_layout_build(const int64_t* counts, int B, int capacity, int32_t* rows, int32_t* cchunk, int32_t* chunks,
                             int32_t* status, void* stream);
int wf3d_packed_layout_build_i32(const int32_t* counts, int B, int capacity, int32_t* rows, int32_t* cchunk,
                                 int32_t* chunks, int32_t* status, void* stream);

/* FORWARD-ONLY encoder (wf3d.infer): the per-point MLP walks the flat row space in blocks and keeps nothing for a
 * backward; these are the two pieces it needs beyond the training forward's entry points.
 *
 * STREAMING 4-way pool.  `state` (wf3d_pool4_stream_state_bytes, 16-byte aligned, device memory) holds per cloud and
 * channel the masked sum, unmasked sum, masked max and unmasked max, and per cloud the number of valid rows seen.
 *   wf3d_pool4_stream_init    sums and counts = 0, maxima = -inf.
 *   wf3d_pool4_stream         folds the rows [r0, r0 + rows) of the flat row space into the state of the clouds they
 *                             belong to; pf [rows, C] (contiguous) and valid [rows] point at row r0.  The cloud of a
 *                             row comes from `offsets`, int32 [B + 1] in device memory (a packed layout's `rows` table;
 *                             b * N for a dense batch), which is never read on the host.  A block may start and end
 *                             anywhere: inside one cloud, across several, over clouds of no rows.  Rows at or past
 *                             offsets[B] (pad and capacity rows) belong to no cloud and are not read.  Every row below
 *                             offsets[B] must be folded exactly once before the finish; the blocks may come in any
 *                             order, the sums are formed in the order they come in.
 *   wf3d_pool4_stream_finish  writes what wf3d_pool4_seg_fwd writes, without the arg-max rows (nothing reads them
 *                             without a backward): mmax (0 where a cloud has no valid row), mavg = masked sum /
 *                             max(count, 1), umean = sum / the cloud's row count, umax — a cloud of no rows pools to
 *                             zeros — each [B, C] with row stride ldo, cnt[b] = max(count, 1), nvalid[b] (optional)
 *                             = count.
 * No floating-point atomics: a block is cut into slices of a height that (rows, C) alone decide, a slice inside one
 * cloud is reduced by one workgroup per 64 channels (C % 64 == 0 and a 16-byte aligned pf: 16 bytes per lane; any other
 * C: one thread per channel), and one owner thread per (cloud, channel) adds the slices to the state in ascending row
 * order, reading the rows of a slice that straddles a cloud boundary itself.  Same calls, same bits. */
size_t wf3d_pool4_stream_state_bytes(int B, int C);
int wf3d_pool4_stream_init(void* state, int B, int C, void* stream);
size_t wf3d_pool4_stream_ws_bytes(int rows, int C);
int wf3d_pool4_stream(const float* pf, const float* valid, const int32_t* offsets, int B, int r0, int rows, int C,
                      void* state, void* ws, size_t ws_bytes, void* stream);
int wf3d_pool4_stream_finish(const void* state, const int32_t* offsets, int B, int C, float* mmax, float* mavg,
                             float* umean, float* umax, int ldo, float* cnt, float* nvalid, void* stream);
/* FIRST LAYER WITHOUT z.  The other instantiation of wf3d_first_layer_fwd's kernel body: its shapes (K <= 8,
 * D % 8 == 0, D <= 1024), its launch and its arithmetic, so h_sx8 = act(LN(x·W^T + b)) is that entry point's h_sx8 bit
 * for bit; z, mu and rs are compiled out (2 KB per row at D = 512 that nothing reads without a backward).  It takes no
 * live-row count. */
int wf3d_first_layer_infer(const float* x, int R, int K, int ldx, const float* W, int ldw, const float* bias, int D,
                           const float* gamma, const float* beta, int act, float eps, void* h_sx8, void* stream);

/* FORWARD-ONLY edge head (wf3d.infer.edge_stream): the edge rows of a layout are walked in blocks through reused
 * buffers; these are the two pieces the walk needs beyond the training forward's entry points.
 *
 * PAIR COMBINE OF A BLOCK.  The kernel body of wf3d_edge_pair_fwd / _fwd_ln (below, "Edge head"), which walks rows
 * e0 + l of the layout and writes at row l (those entry points: e0 = 0), over the edge rows [e0, e0 + n), in its
 * forward-only instantiation: dropout and the stores only a backward reads are compiled out.  Two forms, chosen by the
 * pointers given (anything else is refused):
 *   h_sx8 alone        h = act(LayerNorm(pre)) [n, H] as the sx8 operand of the next Linear (pre = mu = rs = NULL;
 *                      needs gamma, beta, H % 8 == 0 and 16-byte aligned h_sx8 / gamma / beta)
 *   pre, mu, rs alone  pre [n, H], mu [n], rs [n] (h_sx8 = NULL; gamma, beta and act are not read)
 * The arithmetic per row and its order are those entry points': each output equals their rows [e0, e0 + n) bit for bit
 * (drop_p = 0).  e0 is a non-negative multiple of 8, n >= 0 is any count: a block may start in the middle of a sample and
 * end anywhere.  Rows whose esample is negative (a padded layout's tail) get zeros in every output.  Neither esample
 * nor any output is touched at or past row e0 + n.  The calling thread's live-row count is honoured as
 * wf3d_edge_pair_fwd_ln honours it, read as a count over the n rows of THIS block (wf3d_block_live). */
int wf3d_edge_pair_infer(const float* Pa, const float* Pb, const float* cv, const float* wdelta, int wdelta_stride,
                         const int32_t* voff, const int32_t* eoff, const int32_t* esample, int e0, int n, int H, int vd,
                         float eps, const float* gamma, const float* beta, int act, float* pre, float* mu, float* rs,
                         void* h_sx8, void* stream);
/* blive[k] = clamp(*total - k * rows, 0, min(rows, Re - k * rows)) for k < nblocks, int32: the live rows of block k of
 * a walk of Re rows in blocks of `rows`, from the live total in device memory (wf3d_edge_layout's eoff + B), which is
 * never read on the host.  One launch, plain stores. */
int wf3d_block_live(const int32_t* total, int rows, int Re, int nblocks, int32_t* blive, void* stream);

/* ------------------------------------------------------------------------
 * Vertex head tail (VertexPredictor.py:118-127): existence = sigmoid(o[:,:,3]),
 * actual_vertex_counts = sum(existence > 0.5) (int64), o = final_layer output
 * [B, V, vertex_dim >= 4]; backward: d_o[.., k] = d_o_in[.., k] for k < in_dim (d_o_in [B, V, in_dim] contiguous:
 * in_dim = 3 is the gradient of the `vertices` view o[:, :, :3] itself, in_dim = vertex_dim a gradient of o; may be
 * NULL), 0 elsewhere, with dexist*p*(1-p) added into channel 3.
 * ------------------------------------------------------------------------ */
int wf3d_vertex_finalize_fwd(const float* o, int B, int V, int vertex_dim, float* exist, int64_t* counts,
                             void* stream);
int wf3d_vertex_finalize_bwd(const float* exist, const float* dexist, const float* d_o_in, int in_dim, int B, int V,
                             int vertex_dim, float* d_o, void* stream);

/* ------------------------------------------------------------------------
 * Edge head (EdgePredictor.py:91-140, PointCloudToWireframe.py:77-112), batched
 * over samples with COMPACT ragged rows instead of the reference's serial
 * batch-1 loop: sample s owns vertex rows voff[s]..voff[s+1]-1 (its first
 * counts[s] predicted vertices) and edge rows eoff[s]..eoff[s+1]-1 (all pairs
 * i<j in lexicographic order); vsample/esample map a row back to its sample.
 *
 * PADDED layouts (wf3d_edge_layout) are built on the device, so that nothing reads a count on the host: every launch
 * covers the worst case Rv = B*V vertex rows and Re = B*V(V-1)/2 edge rows, and the rows past voff[B] / eoff[B] (the
 * tail) have vsample / esample = -1.  The edge-head kernels below write zeros for a tail row; the attention kernels
 * write only the rows of real samples, so the caller zero-fills ctx / lse / dqkv of a padded layout.
 * ------------------------------------------------------------------------ */
/* counts int64 [B] (device) -> voff / eoff int32 [B+1], vsample int32 [B*V], esample int32 [B*V(V-1)/2] (-1 past the
 * live totals), counts_out int64 [B] = the counts clamped like Python's `[:count]` slicing of V rows (min(c, V) for
 * c >= 0, max(V + c, 0) below) and *width (int64) = max_s c_s(c_s-1)/2.  One launch, plain stores; B <= 4096 and
 * B*V(V-1)/2 must fit in int32. */
int wf3d_edge_layout(const int64_t* counts, int B, int V, int32_t* voff, int32_t* eoff, int32_t* vsample,
                     int32_t* esample, int64_t* counts_out, int64_t* width, void* stream);
/* vd = coordinates per vertex, EdgePredictor(vertex_dim=...), 1..8 (the model uses 3: EdgePredictor.py:19,
 * PointCloudToWireframe.py:38).
 * cv[r,0:vd] = verts[s, r-voff[s], 0:vd]; strides in floats (vertices is a view of [B,V,4]) */
int wf3d_edge_gather_verts(const float* verts, long sample_stride, long vertex_stride, const int32_t* voff,
                           const int32_t* vsample, int Rv, int vd, float* cv, void* stream);
/* dverts[B,V,vd] = scatter of dcv rows, zero for v >= counts[s] */
int wf3d_edge_scatter_dverts(const float* dcv, const int32_t* voff, int B, int V, int vd, float* dverts, void* stream);

/* 8-head self-attention of nn.MultiheadAttention (EdgePredictor.py:41-46,109):
 * qkv[Rv, 3E] packed in_proj output; one workgroup per (head, sample); writes
 * ctx[Rv, E] (heads concatenated, before out_proj) and lse[Rv, heads].  head_dim 64
 * runs QK^T and PV (and the five backward contractions) on fp32 MFMA for any vmax: up
 * to 256 vertices with the sample's rows resident in LDS, beyond that key-tiled with an
 * online softmax (one workgroup per head, sample and 128 rows; option "attn_tiled").
 * Every other head_dim that is a multiple of 4 up to 128 (68..128: hidden 512 / 4 heads,
 * 1024 / 8, 768 / 8) runs key-tiled on fp32 MFMA at any vmax, on kernels of padded width
 * 96 or 128 that neither read nor write past a head's columns.  Head widths up to 60 and
 * above 128 run on VALU kernels that stage up to 256 rows of two operands in LDS: above
 * 128 (and for 68..128 under "attn_tiled" = 0) a call whose rows do not fit the 160 KiB is
 * refused with WF3D_ERR_UNSUPPORTED before anything is launched (width 132: vmax >= 147
 * forward, >= 142 backward).  head_dim % 4 != 0 is refused.  Backward takes the forward's
 * ctx (delta_i = dctx_i · ctx_i); no atomics, so results are bit-reproducible. */
int wf3d_attn_fwd(const float* qkv, const int32_t* voff, int S, int vmax, int E, int heads, float drop_p,
                  uint32_t drop_seed, float* ctx, float* lse, void* stream);
int wf3d_attn_bwd(const float* qkv, const float* dctx, const float* ctx, const float* lse, const int32_t* voff,
                  int S, int vmax, int E, int heads, float drop_p, uint32_t drop_seed, float* dqkv, void* stream);
/* The kernel family that serves such a call under the current options: 0 = VALU, 1 = MFMA with the sample resident in
 * LDS (head_dim 64, vmax <= 256), 2 = MFMA key-tiled (head_dim 64 beyond that, head_dim 68..128 at every vmax);
 * WF3D_ERR_ARG for dims the entry points refuse.  Host only: no device is touched. */
int wf3d_attn_kernel(int E, int heads, int vmax);

/* Split first layer of edge_mlp (EdgePredictor.py:122-137):
 * pre[e,:] = Pa[i,:] + Pb[j,:] + |c_i - c_j| * wdelta  for edge e = (i, j), plus
 * the row's LayerNorm statistics and delta[e] = |c_i - c_j| over the vd coordinates of cv [Rv, vd].  wdelta is column
 * 2H+2vd of edge_mlp.0.weight, read with stride wdelta_stride (= 2H+2vd+1, or 1 for a gathered copy). */
int wf3d_edge_pair_fwd(const float* Pa, const float* Pb, const float* cv, const float* wdelta, int wdelta_stride,
                       const int32_t* voff, const int32_t* eoff, const int32_t* esample, int Re, int H, int vd, float eps,
                       float* pre, float* mu, float* rs, float* delta, void* stream);
/* Same, and also h = drop(act(LayerNorm(pre))) as the sx8 operand of the next Linear (edge_mlp[1..4] of
 * EdgePredictor.py:57-60) from the row the wave still holds: saves wf3d_ln_prep's second read of pre.
 * pre may be NULL: the pre-activation is then not stored at all (2 KB per edge row at hidden 512) and the backward
 * rebuilds it from Pa / Pb with wf3d_edge_pair_ln_bwd below. */
int wf3d_edge_pair_fwd_ln(const float* Pa, const float* Pb, const float* cv, const float* wdelta, int wdelta_stride,
                          const int32_t* voff, const int32_t* eoff, const int32_t* esample, int Re, int H, int vd, float eps,
                          float* pre, float* mu, float* rs, float* delta, const float* gamma, const float* beta, int act,
                          float drop_p, uint32_t drop_seed, void* h_sx8, void* stream);
/* LayerNorm / activation backward of that first edge layer with its pre-activation REBUILT, not read:
 * pre[e, :] = Pa[i, :] + Pb[j, :] + delta[e] * wdelta (the expression the forward kernel evaluated) from the per-vertex
 * tables, which stay L2-resident (V x H per sample).  dh [Re, H] -> dz (may alias dh), dgamma / dbeta (one [2][H]
 * buffer) and wsum[c] = sum_e dz[e, c] * delta[e], the gradient of the distance column of edge_mlp[0].weight
 * (EdgePredictor.py:130-137).  Same arithmetic as wf3d_ln_act_bwd_wsum on a stored pre. */
size_t wf3d_edge_pair_ln_bwd_ws_bytes(int Re, int H);
int wf3d_edge_pair_ln_bwd(const float* dh, const float* Pa, const float* Pb, const float* delta, const float* wdelta,
                          int wdelta_stride, const int32_t* voff, const int32_t* eoff, const int32_t* esample, int Re, int H,
                          const float* mu, const float* rs, const float* gamma, const float* beta, int act, float drop_p,
                          uint32_t drop_seed, float* dz, float* dgamma, float* dbeta, float* wsum, void* ws, size_t ws_bytes,
                          void* stream);
/* dPa[v] / dPb[v] = segmented sums of dpre over the edges where v is i / j, and
 * dcv[v] = sum over incident edges of (dpre[e]·wdelta)(c_v - c_other)/delta[e]
 *          (+ dPa[v]·Wc + dPb[v]·Wd when wcoord != NULL: wcoord[c * wcoord_stride + 0..2vd) = [Wc[c, :] | Wd[c, :]], the
 *          coordinate columns 2H..2H+2vd-1 of edge_mlp[0].weight, EdgePredictor.py:130-137).  dcv is [Rv, vd]. */
int wf3d_edge_pair_bwd(const float* dpre, const float* delta, const float* cv, const float* wdelta,
                       int wdelta_stride, const int32_t* voff, const int32_t* eoff, const int32_t* vsample, int Rv,
                       int H, int vd, float* dPa, float* dPb, float* dcv, const float* wcoord, int wcoord_stride, void* stream);

/* probs[s, j] = sigmoid(logit[eoff[s] + j]) for j < E_s and exactly 0.0 for the padding j >= E_s: the whole padded
 * [B, max_e] output of PointCloudToWireframe.py:103-112 in one pass (no zero-fill first), and its backward. */
int wf3d_edge_prob_fwd(const float* logit, const int32_t* eoff, int B, int max_e, float* probs, void* stream);
int wf3d_edge_prob_bwd(const float* probs, const float* dprobs, const int32_t* eoff, const int32_t* esample, int Re,
                       int max_e, float* dlogit, void* stream);

/* ------------------------------------------------------------------------
 * Row f-1 (next row after the hot path): losses/WireframeLoss.py — the
 * caller of backward.  cost: all B Hungarian cost matrices in one launch
 * (WireframeLoss.py:142-219; the assignment itself stays scipy on the host, :236);
 * terms: SmoothL1 over matched pairs + BCE(existence) + BCE(edges over the common
 * width) and their gradients w.r.t. vertices / existence / edge_probs (:60-104,241-283).
 * losses[4] = {vertex, existence, edge, weighted total}.
 * ------------------------------------------------------------------------ */
int wf3d_loss_cost_matrix(const float* verts, long sample_stride, long vertex_stride, const float* exist,
                          const float* tverts, int Vt, const int64_t* counts, int B, int V, float* cost,
                          void* stream);
/* Hungarian assignment on the device (Jonker-Volgenant shortest augmenting paths, fp64 duals,
 * one wave per sample) — replaces scipy.optimize.linear_sum_assignment + the per-sample
 * .cpu().numpy() sync of WireframeLoss.py:235-236.  col4row[b,p] = column of prediction p;
 * p is matched to a real target iff col4row[b,p] < counts[b].  Any square matrix, V <= 1024.
 * Ties: among the columns of minimal path cost the unassigned one of lowest index, else the lowest index
 * (tests/lsa_model.py states the solver in numpy; the result equals it element for element).
 * Non-finite costs: the solver reads NaN and +inf as FLT_MAX and -inf as -FLT_MAX, so it terminates on every input
 * and col4row[b, :] is always a permutation of 0..V-1 (optimal for the costs so read); it reports nothing.  The loss
 * terms computed from that assignment then carry the NaN of their inputs, as torch's would. */
int wf3d_loss_assign(const float* cost, int B, int V, int32_t* col4row, void* stream);
/* Same result for the wireframe cost (dummy columns >= counts[b] identical per row): solves the count x V rectangular
 * problem "real targets -> distinct predictions, cost c[p,t] - e_p" instead of the padded square one (V <= 64; above
 * that it is wf3d_loss_assign, counts unread).  counts[b] may be any int64 and is clamped to 0..V: a negative count
 * matches nothing (col4row[b, p] = p), one above V is V.  Unmatched predictions get the dummy columns count, count+1,
 * ... in index order.  Same tie rule and the same reading of non-finite costs. */
int wf3d_loss_assign_counts(const float* cost, const int64_t* counts, int B, int V, int32_t* col4row, void* stream);
int wf3d_loss_terms_assigned(const float* verts, long sample_stride, long vertex_stride, const float* exist,
                             const float* edge, int Ep, const float* tverts, int Vt, const float* texist,
                             const float* tlabel, int Et, const int32_t* col4row, const int64_t* counts, int B, int V,
                             float w_vertex, float w_exist, float w_edge, float* dverts, float* dexist, float* dedge,
                             float* losses, void* ws, size_t ws_bytes, void* stream);
/* Same, with the prediction's edge width read from the device (*edge_width, int64: a padded edge head's
 * max_s E_s): the edge term runs over min(*edge_width, Ep, Et) columns, normalised by B x that width, and dedge is 0
 * in the columns past it. */
int wf3d_loss_terms_assigned_ew(const float* verts, long sample_stride, long vertex_stride, const float* exist,
                                const float* edge, int Ep, const float* tverts, int Vt, const float* texist,
                                const float* tlabel, int Et, const int64_t* edge_width, const int32_t* col4row,
                                const int64_t* counts, int B, int V, float w_vertex, float w_exist, float w_edge,
                                float* dverts, float* dexist, float* dedge, float* losses, void* ws, size_t ws_bytes,
                                void* stream);
/* wf3d_loss_terms_assigned (edge_width NULL) or _ew (edge_width given) with the class-balanced / focal edge element
 *   L(p, t) = -( w t (1-p)^gamma max(log p, -100) + (1-t) p^gamma max(log1p(-p), -100) ),   w = edge_pos_weight > 0,
 *   gamma = edge_focal_gamma >= 0 (anything else, NaN and inf included: WF3D_ERR_ARG),
 * dedge its derivative (a clamp that binds has derivative 0), the normaliser unchanged (B x common width).  A side
 * whose coefficient t or 1-t is exactly 0 is not evaluated, and a column with p == t == 0 or p == t == 1 (the padded
 * columns of a ragged batch) contributes exactly 0 and gets gradient exactly 0 at every gamma.  At w = 1, gamma = 0 the
 * call is the plain entry point itself: the same launches, the same bits. */
int wf3d_loss_terms_assigned_bal(const float* verts, long sample_stride, long vertex_stride, const float* exist,
                                 const float* edge, int Ep, const float* tverts, int Vt, const float* texist,
                                 const float* tlabel, int Et, const int64_t* edge_width, const int32_t* col4row,
                                 const int64_t* counts, int B, int V, float w_vertex, float w_exist, float w_edge,
                                 float edge_pos_weight, float edge_focal_gamma, float* dverts, float* dexist, float* dedge,
                                 float* losses, void* ws, size_t ws_bytes, void* stream);
/* Edge labels that follow the matching.  Column k of a prediction row is the pair (p, q) of predicted slots, pair k of
 * the pairs i < j < d_b in lexicographic order; tlabel [B, Et] holds sample b's labels in the pair order of its c_b
 * ground-truth vertices (wf3d.targets.train_targets).  out [B, Ep]:
 *   out[b, k] = tlabel[b, pair_index(min(tp, tq), max(tp, tq), c_b)]   for k < d_b(d_b-1)/2, tp = col4row[b, p] and
 *               tq = col4row[b, q] both in [0, c_b) and different, and that index below Et;
 *             = 0.0 in every other case, and in every column at or past d_b(d_b-1)/2.
 * col4row int32 [B, V]: any assignment (wf3d_loss_assign's, or one with V or a negative value in unmatched slots);
 * counts int64 [B] = c_b and pair_counts int64 [B] = d_b, each clamped to 0..V here; pair_counts NULL: d_b = c_b.
 * One launch over (column chunks, B); every element of out is written exactly once, nothing is read on the host.
 * wf3d.targets.matched_edge_labels states the function in numpy; the result equals it element for element.
 * V <= 1024, B <= 65535, B * Ep and B * Et below 2^31 (else WF3D_ERR_UNSUPPORTED, nothing launched). */
int wf3d_edge_labels_matched(const float* tlabel, int Et, const int32_t* col4row, const int64_t* counts,
                             const int64_t* pair_counts, int B, int V, int Ep, float* out, void* stream);
int wf3d_loss_terms(const float* verts, long sample_stride, long vertex_stride, const float* exist,
                    const float* edge, int Ep, const float* tverts, int Vt, const float* texist,
                    const float* tlabel, int Et, const int32_t* m_pred, const int32_t* m_tgt, const int32_t* m_off,
                    int n_match, int B, int V, float w_vertex, float w_exist, float w_edge, float* dverts,
                    float* dexist, float* dedge, float* losses, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------
 * Row f-2: the step tail of the reference's loop, train.py:141-142 —
 * torch.nn.utils.clip_grad_norm_(model.parameters(), max_norm) followed by torch.optim.Adam.step()
 * (lr, betas, eps, L2 weight_decay; train.py:96) — over ALL tensors in two launches.
 * Tables are HOST arrays of `ntensors` device pointers / element counts.  params[i] == NULL marks a tensor that is only
 * part of the norm and only scaled (the lazily created point_pool_proj, which the reference's optimizer never sees,
 * SURVEY.md §9 Q1).  grads are scaled in place by min(1, max_norm / (norm + 1e-6)) exactly like clip_grad_norm_
 * (max_norm <= 0: no clipping); hyper-parameters are doubles so that 1 - beta, the bias corrections and lr / bc1 are
 * formed in double before their single rounding to fp32, as torch forms them; `step` is the 1-based Adam step of every tensor; total_norm (device scalar, optional)
 * receives the pre-clip global L2 norm.  ws: wf3d_clip_adam_ws_floats() floats.
 * ------------------------------------------------------------------------ */
size_t wf3d_clip_adam_ws_floats(const long* numel, int ntensors);
int wf3d_clip_adam_step(float* const* params, float* const* grads, float* const* exp_avg, float* const* exp_avg_sq,
                        const long* numel, int ntensors, double max_norm, double lr, double beta1, double beta2, double eps,
                        double weight_decay, int step, float* ws, size_t ws_floats, float* total_norm, void* stream);

/* Capturable form (torch.optim.Adam(capturable=True) layout): steps[i] is tensor i's Adam step, a device fp32 scalar
 * (NULL where params[i] is NULL), read by the kernel — steps[i] + 1 is the step applied — and advanced by one after the
 * last Adam launch; every optimised tensor must be at the same step.  lr_dev (device fp32 scalar) replaces lr when
 * non-NULL.  Nothing is read on the host, so a captured launch sequence is right on every replay. */
int wf3d_clip_adam_step_dev(float* const* params, float* const* grads, float* const* exp_avg, float* const* exp_avg_sq,
                            float* const* steps, const long* numel, int ntensors, double max_norm, double lr,
                            const float* lr_dev, double beta1, double beta2, double eps, double weight_decay, float* ws,
                            size_t ws_floats, float* total_norm, void* stream);

/* Grouped form: the same step with the Adam hyper-parameters per PARAMETER GROUP; the norm and the clip coefficient
 * stay global (one clip_grad_norm_ over every tensor of every group and every clip-only tensor).  group[i] in
 * [0, ngroups) is tensor i's group (ignored where params[i] is NULL); lr, beta1, beta2, eps, weight_decay, decoupled
 * and step are HOST arrays of ngroups (at most 16) entries; lr_dev (NULL, or a host array of ngroups device fp32 scalars
 * with NULL entries) replaces lr[k] where non-NULL.  decoupled[k] != 0 selects torch.optim.AdamW's decay for group k:
 * the gradient enters the moments without the decay term and the parameter loses lr * weight_decay * p beside the Adam
 * step, both in one subtraction; 0 is the L2 form of wf3d_clip_adam_step, whose bits a call with equal hyper-parameters
 * in every group reproduces.
 * steps == NULL is the host form: step[k] is the 1-based Adam step of every tensor of group k.  steps != NULL is the
 * capturable form: steps[i] as in wf3d_clip_adam_step_dev, but each tensor's bias corrections come from its own
 * counter, so tensors may be at different steps; `step` is not read.
 * flags: WF3D_ADAM_SKIP_NONFINITE (capturable form only; needs skipped and total_norm) — when the global norm is NaN or
 * infinite, no gradient, parameter, moment or step counter is written, *skipped (device int64) grows by one and
 * total_norm still receives the norm.  The decision is taken on the device from the fp32 sum of squares: finite
 * gradients whose squares overflow fp32 (a norm above 1.8e19) count as non-finite.  Without the flag a NaN norm
 * poisons every tensor, as clip_grad_norm_ does.
 * More than 16 groups: WF3D_ERR_UNSUPPORTED; a group index out of range or the flag without steps: WF3D_ERR_ARG;
 * both before anything is launched. */
#define WF3D_ADAM_SKIP_NONFINITE 1
int wf3d_clip_adam_step_groups(float* const* params, float* const* grads, float* const* exp_avg, float* const* exp_avg_sq,
                               const long* numel, const int* group, float* const* steps, int ntensors, const double* lr,
                               const float* const* lr_dev, const double* beta1, const double* beta2, const double* eps,
                               const double* weight_decay, const int* decoupled, const int* step, int ngroups,
                               double max_norm, int flags, int64_t* skipped, float* ws, size_t ws_floats,
                               float* total_norm, void* stream);

/* The grouped step with averaged weights and the schedules' update count; every other argument is
 * wf3d_clip_adam_step_groups' own, and with ema == NULL and schedule_step == NULL so are the launches and the bits.
 * ema (NULL, or a host array of ntensors device pointers with NULL entries): tensor i's exponential moving average, fp32
 * of numel[i] elements.  In the pass that stores the new parameter value p', ema' = fmaf(1 - d, p' - ema, ema) with
 * d = ema_decay[group[i]] (host array of ngroups doubles in [0, 1); a tensor with an average needs d > 0) and 1 - d
 * rounded once from double.  WF3D_ADAM_EMA_WARMUP: d = min(ema_decay, (1 + n) / (10 + n)), formed in double, where n is
 * the tensor's Adam step before this update (capturable form: steps[i]; host form: step[k] - 1).  p, g, m, v and the
 * norm are those of the step without the average, bit for bit; lr = 0 still moves the average; a skipped step leaves
 * it alone; clip-only tensors have none.  An average costs 8 B per parameter on top of 32, and a launch with an ema
 * table carries 40 tensors instead of 48 (the partial sums of the norm do not move).
 * schedule_step (capturable form only, may be NULL): a device int64 that grows by one in a step that advances at least
 * one Adam counter — not in a skipped step, not in a step of clip-only tensors alone — in the launch that advances
 * those counters.  It is what wf3d_lr_schedule reads. */
#define WF3D_ADAM_EMA_WARMUP 2
int wf3d_clip_adam_step_ema(float* const* params, float* const* grads, float* const* exp_avg, float* const* exp_avg_sq,
                            float* const* ema, const long* numel, const int* group, float* const* steps, int ntensors,
                            const double* lr, const float* const* lr_dev, const double* beta1, const double* beta2,
                            const double* eps, const double* weight_decay, const int* decoupled, const double* ema_decay,
                            const int* step, int ngroups, double max_norm, int flags, int64_t* skipped,
                            int64_t* schedule_step, float* ws, size_t ws_floats, float* total_norm, void* stream);

/* Learning-rate schedules on the device: one launch, one thread per group, writes
 * last_lr[k] = float(lr[k] * fw * fd) (formed in double, rounded once) for every group with write[k] != 0, from
 * t = *schedule_step, the number of updates applied so far; the step entry points read it through lr_dev[k].  All
 * tables are HOST arrays of ngroups (at most 16) entries; milestones has 8 per group, of which nmilestones[k] count.
 *   fw = warmup_start + (1 - warmup_start) t / warmup_steps   for t < warmup_steps, else 1
 *   u  = max(t - warmup_steps, 0),  T = decay_steps,  x = min(u, T) / T
 *   fd = 1 (CONSTANT);  min_factor + (1 - min_factor) (1 + cos(pi x)) / 2 (COSINE);  1 + (min_factor - 1) x (LINEAR);
 *        max(gamma^u, min_factor) (EXPONENTIAL);  gamma^(number of milestones <= u) (MULTISTEP)
 * Past T, COSINE and LINEAR stay at min_factor.  warmup_steps 0 with CONSTANT is "no schedule": float(lr[k]).
 * Refused with WF3D_ERR_ARG before the launch: warmup_steps < 0, decay_steps < 1 where COSINE or LINEAR read it,
 * warmup_start or min_factor outside [0, 1], gamma outside (0, 1] where it is read, more than 8 or decreasing
 * milestones, an unknown decay. */
#define WF3D_LR_CONSTANT 0
#define WF3D_LR_COSINE 1
#define WF3D_LR_LINEAR 2
#define WF3D_LR_EXPONENTIAL 3
#define WF3D_LR_MULTISTEP 4
int wf3d_lr_schedule(const double* lr, const long* warmup_steps, const double* warmup_start, const int* decay,
                     const long* decay_steps, const double* min_factor, const double* gamma, const long* milestones,
                     const int* nmilestones, const int* write, int ngroups, const int64_t* schedule_step, float* last_lr,
                     void* stream);

/* Parameters and averages change places, element for element: ntensors pairs of numel[i] fp32 values each (host
 * tables of device pointers, no NULL entries).  Two calls are the identity, bit for bit.  Capturable. */
int wf3d_ema_swap(float* const* params, float* const* ema, const long* numel, int ntensors, void* stream);

/* ------------------------------------------------------------------------
 * Device-side dropout seeds (wf3d/random.py).  state = {key, counter} (uint64, device).  wf3d_dropout_draw: one thread
 * writes words[0..4] = s + k * 0x9E3779B9 (k = 0..4; words[k] for k >= 1 are EdgeFn's per-site seeds) with
 * s = low 32 bits of splitmix64 at position counter + 1 of the key's stream, then advances the counter.
 * wf3d_set_dropout_seed_words (thread-local, host only): while `words` is non-NULL, every `drop_seed` argument of a
 * launch with drop_p > 0 on the calling thread (wf3d_gemm_t.drop_seed included) is an index into these device words,
 * loaded by the kernel at run time; NULL restores seeds by value.
 * ------------------------------------------------------------------------ */
int wf3d_dropout_draw(uint64_t* state, uint32_t* words, void* stream);
int wf3d_set_dropout_seed_words(const uint32_t* words);

/* ------------------------------------------------------------------------
 * LIVE ROW COUNT.  A padded edge layout runs every edge-row launch at the worst case B*V(V-1)/2 rows, a packed batch with
 * a capacity every per-point launch at `capacity` rows.  While the calling
 * thread has set a live-row count, wf3d_set_live_rows(rows) with rows -> one int32 in DEVICE memory (wf3d_edge_layout's
 * eoff + B; wf3d_packed_layout_build's rows + B), the launches listed below skip the tail.  The pointer is a kernel argument and the value is read by the
 * kernel at entry, never on the host: a captured graph stays valid when the value changes between replays.  NULL
 * clears it.  Thread-local, host only, like wf3d_set_dropout_seed_words; a side stream driven from the same thread
 * is covered.
 *
 * With R the launch's host-side row extent (the worst case, as without a count), live = clamp(*rows, 0, R) and
 * R256 = min(R, 256 * ceil(live / 256)):
 *   - no row >= R256 of a row-indexed operand is read, no row >= R256 of a row-indexed output is written;
 *   - rows [0, R256) are read and written exactly as without a count, the dead rows [live, R256) included (zeros from
 *     the pair kernel, bias-only values after a forward GEMM, exact zeros in every backward dz);
 *   - reductions over rows (wf3d_colsum, the dgamma / dbeta / dbias / wsum of the LayerNorm backward, the column sums
 *     of wf3d_rowdot_act_bwd, the K dimension of the TN weight-gradient GEMMs) cover [0, R256) only;
 *   - grids, kernel choice, split-K plans and workspace sizes stay the host-side worst-case ones; slabs and partial
 *     sums are folded in the same order, a workgroup whose rows lie past R256 contributes an exact zero.
 * So every result in rows < R256 is bit-identical to the same launch without a count, and every reduced result is
 * whenever the skipped rows of the reduced operand were zeros (every backward tail of a padded edge head is).
 * live = 0 is legal: nothing is read, row outputs are untouched, reduced outputs are exact zeros.
 * 256: every tile height and K slice of these kernels divides it, so no kernel needs a partial-tile path.
 *
 * Honoured by (rows = the dimension named):
 *   wf3d_gemm_split, wf3d_gemm_bf16            M, every kernel form and the split-K combine
 *   wf3d_gemm_split_tn, wf3d_gemm_bf16_tn      K, every kernel form (Mo, No are weight dimensions)
 *   wf3d_ln_prep, wf3d_ln_act_bwd, wf3d_ln_act_bwd_wsum, wf3d_edge_pair_ln_bwd, wf3d_rowdot_act, wf3d_rowdot_act_bwd,
 *   wf3d_colsum                                R / Re
 *   wf3d_edge_pair_fwd, wf3d_edge_pair_fwd_ln, wf3d_edge_prob_bwd      Re
 *   wf3d_edge_pair_infer                       n, the rows of the block (a block-local count)
 *   wf3d_split_rows                            R (rows of the output)
 *   wf3d_split_transpose                       R (rows of the input), both the fp32 / prologue and the in_sx8 form.  Its
 *                                              output is [C, R]: the input's rows are its COLUMNS, the reduction
 *                                              dimension of the NT GEMM that consumes a pair of transposed operands.
 *                                              No input row >= R256 (nor its mu / rs) is read, the columns < R256 are
 *                                              written as without a count, and the columns [R256, R) are written as
 *                                              exact zeros.  The caller runs that GEMM WITHOUT a count (its rows are a
 *                                              weight dimension): the zero columns add exact zeros in its unchanged
 *                                              split-K order, as the zero backward tail does without a count.
 *   wf3d_first_layer_fwd, _fwd_drop            R, every kernel form: z, mu, rs and h_sx8 are written for rows < R256 only
 *   wf3d_ln_act_bwd_first, _first_drop         R; dgamma / dbeta / dbias and dW are sums over [0, R256)
 *   wf3d_point_valid                           M
 *   wf3d_pool4_seg_bwd, wf3d_pool4_seg_bwd_sx8 M_pad, with the count in rows of the packed batch (the layout's
 *                                              rows[B]): a pad chunk (-1, 0, r0, r1) zero-fills [r0, min(r1, R256)).
 *                                              The clouds' chunks lie below the live total and run as without a count.
 * wf3d_pool4_seg_fwd reads rows through the clouds' chunks only and touches no pad row with or without a count, as
 * wf3d_edge_pair_bwd and wf3d_edge_prob_fwd reach edge rows through eoff only and touch no tail row with or without
 * a count.  EVERY OTHER entry point ignores the count and cannot see it: wf3d_gemm (the fp32 routes), the attention
 * and skinny kernels, wf3d_row_stats, wf3d_ln_act_apply, wf3d_split_rows_multi (weights), the
 * per-vertex launches.  The caller clears the count around launches over other rows (the
 * honouring entry points apply it to whatever rows they are given).
 * ------------------------------------------------------------------------ */
int wf3d_set_live_rows(const int32_t* rows);

/* Training-step meter (reference train.py:145-157: total_loss.item() twice and a host copy of sample 0's vertices on EVERY
 * step, for the loss history, the best loss and a monitoring RMSE).  One small launch per step folds them into a
 * device-resident record; the loop copies it back only when it logs.
 *   state[0] = steps recorded, [1] = best total loss, [2] = best vertex RMSE, [3..7] = last total / vertex / existence /
 *   edge loss and RMSE, [8 .. 8 + capacity) = ring of the last `capacity` total losses (step t at 8 + t % capacity);
 *   the caller zeroes state[0] once.  RMSE = sqrt(mean((pred - target)^2)) over the first count0[0] (<= max_v) vertices
 *   x 3 coordinates of sample 0; pred_stride / target_stride = floats between consecutive vertices.
 *   vertex_loss / existence_loss / edge_loss / count0 may be NULL (recorded as 0 / count = max_v). */
int wf3d_meter_update(const float* total, const float* vertex_loss, const float* existence_loss, const float* edge_loss,
                      const float* pred_vertices, long pred_stride, const float* target_vertices, long target_stride,
                      const int64_t* count0, int max_v, float* state, int capacity, void* stream);

/* Training metrics (wf3d.meter.WireframeMeter): batch-wide quality counters from the assignment the loss has solved
 * (col4row of wf3d_loss_assign, int32 [B, V]), in two launches with no atomics: the same inputs give the same bits.
 * verts / exist / edge / tverts / texist / tlabel / counts as wf3d_loss_terms_assigned takes them.  With
 * c_b = clamp(counts[b], 0, min(V, Vt)):
 *   matched pair   slot p of sample b with 0 <= col4row[b, p] < c_b, its target t = col4row[b, p]; every other value
 *                  (negative, >= c_b) leaves the slot unmatched, and the pairs are counted, not assumed to be c_b.
 *                  d2 = ((dx dx + dy dy) + dz dz) in fp64 from the fp32 coordinates, each product and sum rounded;
 *                  sum_sq += d2, sum_dist += sqrt(d2), n_within += (d2 <= double(distance_thresh)^2).
 *   existence      over all B * V slots: predicted exist > 0.5f, label texist > 0.5f -> ex_tp, ex_fp, ex_fn;
 *                  count_abs_err += |#(exist[b] > 0.5f) - c_b| per sample.
 *   edges          over the first w = min(Ep, Et) columns, or min(*edge_width, Ep, Et) with edge_width (a padded edge
 *                  head's device width, read when the kernels run): predicted edge > edge_threshold, label tlabel >
 *                  0.5f -> ed_tp, ed_fp, ed_fn.  Columns at or past w are not read.
 * Comparisons with NaN are false: the integer counters stay finite, the two sums carry the NaN.
 * state [2][13] fp64 (8-byte aligned): row 0 is written with this batch, row 1 grows by it (the caller zeroes row 1 to
 * reset); columns updates (1 per call), n_samples (B), n_pairs, sum_sq, sum_dist, n_within, ex_tp, ex_fp, ex_fn,
 * count_abs_err, ed_tp, ed_fp, ed_fn.  Counts held in fp64 are exact to 2^53.
 * ws: wf3d_train_metrics_ws_bytes(B, Ep) bytes, 16-byte aligned (one record per sample and per 2048 edge columns).
 * V <= 1024, B <= 65535, B * Ep and B * Et below 2^31, else WF3D_ERR_UNSUPPORTED; B, V, Vt >= 1. */
size_t wf3d_train_metrics_ws_bytes(int B, int Ep);
int wf3d_train_metrics(const float* verts, long sample_stride, long vertex_stride, const float* exist, const float* edge,
                       int Ep, const float* tverts, int Vt, const float* texist, const float* tlabel, int Et,
                       const int32_t* col4row, const int64_t* counts, const int64_t* edge_width, int B, int V,
                       float edge_threshold, float distance_thresh, double* state, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------
 * Row f-3: the input pipeline, datasets/building3d.py:95-158.  Clouds are parsed once, normalised once on
 * the device in float64 (the raw coordinates are UTM metres: colour / 256 for columns [color_lo, color_hi), centroid and
 * max-norm of xyz, :101-121) and stay resident; every batch is then ONE gather kernel: random rows (:127), flips and the
 * rotation about z (:130-145) applied in float64 and rounded to fp32 once (:158).  The random choices [B, P] and
 * aug[b] = {flip_x (+-1), flip_y (+-1), cos t, sin t} come from the host's numpy RNG in the reference's draw order.
 * Packed layout: cloud i owns rows first[i] .. first[i+1]-1 of raw / out ([rows, C] float64).
 * ------------------------------------------------------------------------ */
int wf3d_cloud_normalize(const double* raw, const long* first, int nclouds, int C, int color_lo, int color_hi, int normalize,
                         double* out, double* centroid, double* max_distance, void* stream);
int wf3d_cloud_sample(const double* norm, const long* first, const int* cloud, const int* choice, const double* aug, int B,
                      int P, int C, float* out, void* stream);
/* Packed batches from the resident clouds (wf3d.packed, "PACKED batches, capacity form"): two launches fill the static
 * buffers of a captured step.  Both read one PARAMETER BLOCK in device memory, 8-byte aligned, B * 40 + 4 bytes:
 *     double aug[B][4]         {flip_x (+-1), flip_y (+-1), cos t, sin t} of sample b          at byte 0
 *     int    cloud[B]          the resident cloud of sample b, 0 .. nclouds-1                  at byte 32 * B
 *     int    out_first[B + 1]  sample b's first output row; out_first[0] = 0,                  at byte 36 * B
 *                              out_first[b+1] - out_first[b] = first[cloud[b]+1] - first[cloud[b]], out_first[B] <= capacity
 * The host fills it (numpy draws in the reference's order) and copies it up, or wf3d_cloud_epoch_params (below) writes it
 * on the device; the launches take only its address, so a
 * captured graph replays them on whatever block is there.  1 <= B <= 4096.
 * wf3d_cloud_pack: points [capacity, C] fp32 — cloud[b]'s rows in file order at rows out_first[b] .. out_first[b+1]-1, each
 *   with the flips and the z-rotation of wf3d_cloud_sample (float64, one rounding), rows out_first[B] .. capacity-1 exact
 *   zeros — and point_counts[b] = the rows of cloud[b].  Every element of both is written, by plain stores of this one
 *   launch.  C = 8 moves 16 bytes per access (norm and points 16-byte aligned); other C take a row per lane.  A row whose
 *   cloud index or position falls outside the resident clouds (a block that breaks the rules above) is written as zeros.
 * wf3d_wireframe_targets: wf3d.targets.train_targets(..., full_width=True) of the samples' wireframes.  Resident:
 *   wf_vertices [sum c, 3] float64 (centred and scaled like the clouds), wf_edges [sum e, 2] int32 vertex indices inside
 *   their wireframe, vfirst / efirst [nclouds + 1] row offsets.  Writes every element of vertices [B, V, 3] (c_s vertices,
 *   augmented like the points, then zeros), vertex_existence [B, V], vertex_counts [B] = c_s and edge_labels
 *   [B, V(V-1)/2]: 1.0 at pair (i, j)'s position among the pairs of c_s vertices for every edge with 0 <= i < j < c_s,
 *   0.0 elsewhere.  The host refuses c_s > V before the launch; the kernel would treat such a sample as c_s = V.
 * wf3d_cloud_sample_dev: the FIXED-SIZE batch of the same block, sampled in the kernel: points [B, P, C] fp32 with
 *   points[b, p, :] = fp32(augment(norm[first[cloud[b]] + idx(b, p), :])), the flips and the z-rotation of
 *   wf3d_cloud_sample (float64, one rounding), and idx(b, .) = wf3d.sampling.choice_indices(seed_words[0], b, n_b, P),
 *   n_b the rows of cloud[b]: P distinct rows when n_b >= P (a keyed Feistel permutation, cycle-walked), P independent
 *   uniform rows when n_b < P — np.random.choice(n_b, P, replace=n_b < P) in distribution, another random stream.
 *   seed_words: DEVICE memory, 4-byte aligned; word 0 is read by the kernel at run time (wf3d_dropout_draw on a generator
 *   state of the caller's own writes it), so a captured launch samples afresh on every replay.  out_first is ignored (the
 *   host writes out_first[b] = b * P).  Every element of points is written, by plain stores of this one launch; a sample
 *   whose cloud index is outside 0 .. nclouds-1 or whose cloud is empty is written as zeros.  1 <= P, B * P < 2^31;
 *   C = 8 moves 16 bytes per access (norm and points 16-byte aligned), other C take a row per lane. */
int wf3d_cloud_pack(const double* norm, const long* first, int nclouds, const void* params, int B, int capacity, int C,
                    float* points, int64_t* point_counts, void* stream);
int wf3d_cloud_sample_dev(const double* norm, const long* first, int nclouds, const void* params, const uint32_t* seed_words,
                          int B, int P, int C, float* points, void* stream);
int wf3d_wireframe_targets(const double* wf_vertices, const int32_t* wf_edges, const long* vfirst, const long* efirst, int nclouds,
                           const void* params, int B, int V, float* vertices, float* vertex_existence, int64_t* vertex_counts,
                           float* edge_labels, void* stream);
/* FARTHEST-POINT SAMPLING: wf3d_cloud_sample_dev's fixed-size batch — the same parameter block, word 0 of the same
 * seed_words, both read in device memory at run time (a captured launch samples afresh on every replay), out_first
 * ignored — with the rows chosen by distance: points[b, p, :] = fp32(augment(norm[first[cloud[b]] + idx(b, p), :])),
 * idx(b, .) = wf3d.sampling.fps_indices(seed_words[0], b, xyz of cloud[b], P), bit for bit:
 *     start    = mulhi(fmix32(key ^ 0xB5297A4D), n_b), the offset `a` of the random sampler: one start per (word, sample)
 *     a round  = every row's d (+inf at first; -1 once picked) lowered to r = ((dx dx + dy dy) + dz dz) from the row just
 *                picked where r < d, then the row of the largest d, the LOWEST index among equals; float64 on columns 0..2
 *                of `norm` BEFORE the augmentation (flips and the z-rotation are isometries), every operation rounded on
 *                its own, no fma.  A NaN r lowers nothing, so a row with non-finite coordinates is picked early.
 *     idx(b, p) = order[p mod n_b] over min(n_b, P) rounds: a cloud shorter than P repeats its order cyclically.
 * The flips and the rotation are wf3d_cloud_sample's (float64, one rounding) through wf3d_cloud_sample_dev's gather: C = 8
 * moves 16 bytes per access (norm and points 16-byte aligned), other C take a row per lane.  idx_out: int32 [B, P] or
 * NULL; receives idx(b, p).  Every element of points, and of idx_out when given, is written by plain stores of this one
 * launch; a sample whose cloud index is outside 0 .. nclouds-1, whose cloud is empty or longer than max_rows is written
 * as zeros, its idx_out row too.
 * One workgroup per sample and no synchronisation between workgroups; P - 1 dependent rounds of one barrier each.
 * max_rows: the rows of the longest resident cloud (the caller knows it; `first` is device memory).  It sizes the
 * workgroup (256 threads up to 2048 rows, 512 up to 4096, else 1024); clouds of at most WF3D_FPS_REG_ROWS rows keep
 * their coordinates and d in registers for all rounds.  max_rows above it: ws holds d and the order of the longer clouds,
 * wf3d_cloud_sample_fps_ws_bytes(B, max_rows) bytes (0 up to WF3D_FPS_REG_ROWS), 8-byte aligned, and those clouds read
 * their coordinates again every round — that tier is correct and NOT tuned.
 * 1 <= B <= 4096, 1 <= P, B * P < 2^31, 1 <= max_rows < 2^31, else WF3D_ERR_ARG before any launch. */
#define WF3D_FPS_REG_ROWS 8192
size_t wf3d_cloud_sample_fps_ws_bytes(int B, long max_rows);
int wf3d_cloud_sample_fps(const double* norm, const long* first, int nclouds, const void* params, const uint32_t* seed_words,
                          int B, int P, int C, float* points, int32_t* idx_out, long max_rows, void* ws, size_t ws_bytes,
                          void* stream);
/* RESIDENT EPOCHS: the parameter block above and the seed words of wf3d_cloud_sample_dev, written ON THE DEVICE from
 * state = {uint64 key, uint64 t} (device memory, 8-byte aligned; t = the batches produced so far), so that a captured
 * graph of this launch and the launches above walks shuffled, rank-sharded, augmented epochs with no host work between
 * replays.  wf3d.sampling.epoch_batch is the specification, bit for bit.  With mix64(key, n) = wf3d_dropout_draw's
 * splitmix64 step, S = D / (world * B) steps per epoch (the last partial batch is dropped), e = t / S, s = t % S and
 * g = s * world * B + rank * B + b the global slot of sample b:
 *     cloud[b]  = members[order_e[g]], order_e = wf3d.sampling.choice_indices(low32(mix64(key, e)), 0, D, D): a permutation
 *                 of 0 .. D-1 per epoch; members = int32 [D] resident cloud indices (device memory)
 *     aug[b]    = {1, 1, 1, 0} without `augment`, else with c = e * 2^32 + g: flip_x = -1 iff bit 63 of
 *                 za = mix64(key ^ 0x6A09E667F3BCC908, c), flip_y the same on bit 62, and cos / sin of
 *                 t_rot = u * (pi / 18) - pi / 36, u = (mix64(key ^ 0xBB67AE8584CAA73B, c) >> 11) * 2^-53, as the fixed
 *                 polynomials of wf3d.sampling.epoch_cos_sin, every operation rounded on its own (no fma)
 *     out_first = b * P for the fixed-size form (P >= 1); P = 0, the packed form: the exclusive prefix sum of the rows of
 *                 cloud[0 .. B-1] (a cloud index outside 0 .. nclouds-1 counts no rows)
 *     seed_words[k] = low32(mix64(key ^ 0x3C6EF372FE94F82B, t * world + rank)) + k * 0x9E3779B9, k = 0 .. 4
 * then t += 1.  Slots and augmentation depend on (e, g) only: the ranks' batches of a step are disjoint and their union
 * is the batch of one rank with batch world * B; the seed words are per (step, rank).  One workgroup: every thread
 * reads the state, a barrier, one thread stores t + 1; every byte of the block and of the five words is written by plain
 * stores.  1 <= D < 2^31, 1 <= B <= 4096 (WF3D_ERR_UNSUPPORTED above), 0 <= rank < world, world * B <= D, B * P < 2^31.
 * The caller sees to it that no batch of `members` breaks the rules of the launches behind it (row capacity, V). */
int wf3d_cloud_epoch_params(uint64_t* state, const int32_t* members, int D, const long* first, int nclouds, int B, int world,
                            int rank, int P, int augment, void* params, uint32_t* seed_words, void* stream);
/* THE AUGMENTATION EXTENSION of the sampled forms: a random scale, per-point jitter and random point dropout inside the
 * gather — still one launch, float64 and one rounding.  wf3d.sampling.augment_point / jitter_noise / dropped are the
 * specification, bit for bit.  The EXTENSION BLOCK `ext` is float64 [B, 8] in device memory, 8-byte aligned, BESIDE the
 * parameter block (whose layout does not change): per sample {sx, sy, sz, sigma, clip, drop, 0, 0}.  The host fills it,
 * or wf3d_cloud_epoch_params_ext writes it.  With (key, key2) the row sampler's keys of sample b under seed_words[0]
 * and K = key * 2^32 | key2, output row p of sample b is
 *     dropped    iff p >= 1 and (mix64(K ^ 0x1F83D9ABFB41BD6B, p) >> 11) * 2^-53 < drop; p_eff = 0 if dropped, else p: a
 *                dropped row is an exact copy of output row 0 (row 0 is never dropped)
 *     its source idx(b, p_eff) of the plain entry point, and (xr, yr, z) that entry point's float64 values BEFORE its rounding
 *     g_k      = (double)(S_k - 131070) * 0x1.bb67ae8584caap-16, S_k the sum of the four 16-bit fields of
 *                mix64(K ^ 0x9B05688C2B3E6C1F, 3 * p_eff + k), k = 0, 1, 2: Irwin-Hall of four, mean 0, variance 1,
 *                |g| <= 3.4641, no transcendental
 *     j_k      = min(max(sigma * g_k, -clip), clip)
 *     x' = xr * sx + j_0, y' = yr * sy + j_1, z' = z * sz + j_2: every operation rounded on its own (no fma), then ONE
 *                rounding to fp32; sigma == 0 adds nothing, so a -0.0 keeps its sign.  Columns 3 and up are the plain form's.
 * An identity row {1, 1, 1, 0, inf, 0} gives the plain entry point's bits.  No value of `ext` moves an address: it
 * changes arithmetic and replaces p by 0, nothing else.  In a block the host did not build, a NaN scale, sigma or clip
 * gives NaN coordinates and a NaN drop drops nothing; a dead sample is still all zeros.
 * wf3d_cloud_sample_dev_ext / wf3d_cloud_sample_fps_ext: the plain argument lists plus `ext` (NULL: WF3D_ERR_ARG), the
 *   same kernels with the extension compiled in.  At C = 8, x, y and z sit in the even lane of a row's pair; the odd
 *   lane and every 16-byte access are the plain form's.  Farthest-point sampling leaves its rounds alone — distances are
 *   measured on the resident coordinates, unscaled (an anisotropic scale is no isometry: accepted) — takes idx(b, 0)
 *   for a dropped row and reports that index in idx_out.
 * wf3d_wireframe_targets_ext: vertices = the plain form's float64 values times (sx, sy, sz), each product rounded on its
 *   own, then one rounding to fp32; no jitter, no dropout.  vertex_existence, vertex_counts and edge_labels are the
 *   plain form's bits, and so are the vertices where sx = sy = sz = 1.
 * wf3d_cloud_epoch_params_ext: wf3d_cloud_epoch_params, which also writes every byte of `ext` — still one workgroup, one
 *   launch, t += 1 once.  cfg: HOST memory, 8 doubles {lo, hi, anisotropic (0 or 1), sigma, clip, max_dropout, 0, 0},
 *   held to wf3d.sampling.check_augment: finite 0 < lo <= hi, finite sigma >= 0, clip > 0 (inf: no clip), max_dropout
 *   in [0, 1], else WF3D_ERR_ARG before any launch.  With c = e * 2^32 + g as for the flips
 *   (wf3d.sampling.epoch_augment_ext):
 *     s_k  = lo + u_k * (hi - lo), u_k = (mix64(key ^ (0xA54FF53A5F1D36F1 + k), c) >> 11) * 2^-53; k = 0, 1, 2 when
 *            anisotropic, else k = 0 for the three axes
 *     drop = u_d * max_dropout, u_d from 0x510E527FADE682D1; sigma and clip copied
 *   so scale and dropout ratio depend on (epoch, global slot) only and are world-size invariant; jitter and the dropped
 *   rows are keyed by seed_words[0] and the LOCAL b, per (step, rank) like the row choice, and are not. */
int wf3d_cloud_sample_dev_ext(const double* norm, const long* first, int nclouds, const void* params, const uint32_t* seed_words,
                              int B, int P, int C, float* points, const double* ext, void* stream);
int wf3d_cloud_sample_fps_ext(const double* norm, const long* first, int nclouds, const void* params, const uint32_t* seed_words,
                              int B, int P, int C, float* points, int32_t* idx_out, long max_rows, void* ws, size_t ws_bytes,
                              const double* ext, void* stream);
int wf3d_wireframe_targets_ext(const double* wf_vertices, const int32_t* wf_edges, const long* vfirst, const long* efirst, int nclouds,
                               const void* params, int B, int V, float* vertices, float* vertex_existence, int64_t* vertex_counts,
                               float* edge_labels, const double* ext, void* stream);
int wf3d_cloud_epoch_params_ext(uint64_t* state, const int32_t* members, int D, const long* first, int nclouds, int B, int world,
                                int rank, int P, int augment, void* params, uint32_t* seed_words, const double* cfg, double* ext,
                                void* stream);
/* HOST function: the numbers of a whitespace-separated text file (.xyz: 8 per row; np.loadtxt, :98) into out[0..max_vals);
 * returns the count in the file (call again with a larger buffer if > max_vals), -1 unreadable, -2 not a number: a token
 * is every character up to whitespace, `#` or the end, and the whole of it must be one decimal number, inf or nan, as
 * for np.loadtxt (`3.4.5`, `1.0-2.0`, `1e5x`, `1,2,3` and hexadecimal forms such as `0x10` are refused). */
long wf3d_parse_floats(const char* path, double* out, long max_vals);
/* Same (`#` comments skipped, C-locale numbers; \n, \r\n and a lone \r end a row), and *ncols = values per row — np.loadtxt's second dimension;
 * -3 if two non-empty rows hold different numbers of values. */
long wf3d_parse_table(const char* path, double* out, long max_vals, long* ncols);

/* ------------------------------------------------------------------------
 * Row f-4: evaluation post-processing behind the path, evaluate.py:74-110 and
 * eval/ap_calculator.py:8-36.
 * wf3d_edge_endpoints: for every sample s and every candidate edge e = (i < j < counts[s]) in the model's lexicographic
 * order: keep[s, e] = probs[s, e] > threshold (:79) and edge_vertices[s, e] = the two predicted end points, higher z first
 * (:88-89; equal z: vertex j first) — all samples in one launch, so the host needs one copy instead of one per sample.
 * verts strides in floats (the `vertices` output is a view).  Entries e >= E_s are left untouched.
 * wf3d_hausdorff_lines: out[n, m] = max(h(P_n, T_m), h(T_m, P_n)) over `sample_points` (<= 32) equidistant points per
 * segment, point k = start + w_k * diff with np.linspace's weights; float64.
 *
 * wf3d_edge_compact: the same selection as a stable stream compaction, so that what the host reads scales with the KEPT
 * edges.  Candidate e of sample s is kept iff e < c_s (c_s - 1) / 2, e < max_e and probs[s, e] > threshold (a NaN or a
 * value equal to the threshold is not kept), c_s = counts[s] clamped to 0 .. V.  koff[B + 1] = exclusive prefix of the
 * per-sample kept counts (koff[B] = K); packed over k in [0, K), in sample order and within a sample in increasing e:
 * pairs[k] = (i, j), i < j; seg[k] = the two end points, higher z first (equal z: vertex j first); kprob[k] = the
 * probability.  pairs / seg / kprob hold B * max_e rows (the worst case); rows k >= K are left untouched.  Three
 * launches (kept count per 256-candidate chunk, one scan over the B * ceil(max_e / 256) chunk counts, placement by wave
 * ballot ranks): no atomics, the same bits on every run.  ws: wf3d_edge_compact_ws_bytes(B, max_e) bytes.
 * B <= 65535 and B * max_e < 2^31, else WF3D_ERR_UNSUPPORTED; B = 0, V < 2 or max_e = 0 write koff = 0 and launch nothing.
 * wf3d_hausdorff_lines_batch: the [n_s, m_s] matrices of wf3d_hausdorff_lines for every sample of a batch in one launch,
 * n_s = koff[s + 1] - koff[s] predicted segments of seg [K, 2, 3] (wf3d_edge_compact's) against m_s = loff[s + 1] -
 * loff[s] label segments of lseg [L, 2, 3], both float32: diff = end - start is an fp32 subtraction (the common dtype
 * of float32 predictions and labels), widened to float64 afterwards.  Sample s's matrix is written row-major at
 * out + ooff[s]; ooff[B + 1] = exclusive prefix of n_s * m_s (the caller's, device memory), max_pairs = max_s n_s * m_s
 * sizes the grid.  Samples with n_s * m_s = 0 write nothing.  B <= 65535.
 * ------------------------------------------------------------------------ */
int wf3d_edge_endpoints(const float* verts, long sample_stride, long vertex_stride, const int32_t* counts, const float* probs,
                        int B, int V, int max_e, float threshold, float* edge_vertices, unsigned char* keep, void* stream);
int wf3d_hausdorff_lines(const double* p_start, const double* p_diff, const double* t_start, const double* t_diff, int N, int M,
                         int sample_points, double* out, void* stream);
size_t wf3d_edge_compact_ws_bytes(int B, int max_e);
int wf3d_edge_compact(const float* verts, long sample_stride, long vertex_stride, const int32_t* counts, const float* probs,
                      int B, int V, int max_e, float threshold, int32_t* koff, int32_t* pairs, float* seg, float* kprob,
                      void* ws, size_t ws_bytes, void* stream);
int wf3d_hausdorff_lines_batch(const float* seg, const int32_t* koff, const float* lseg, const int32_t* loff,
                               const int64_t* ooff, int B, long max_pairs, int sample_points, double* out, void* stream);

/* ------------------------------------------------------------------------
 * Wireframe decoding (csrc/evalpost.hip; the specification, stated in numpy, is wf3d/decode.py and the kernel gives its
 * values exactly): one forward pass -> per sample a wireframe of vertices that exist, are distinct and are connected.
 * The reference has no such step: it hands all V slots to its metrics.
 * Inputs: verts [B, V, 3] (strides in floats, unit inner stride), exist [B, V] with element stride exist_stride and
 * sample stride V * exist_stride (a column of a [B, V, k] tensor passes as it is), counts [B], probs [B, max_e] in the
 * model's lexicographic pair order over the first c_s = clamp(counts[s], 0, V) slots.
 *   1. slot i is alive iff i < c_s, its coordinates are finite, its existence is not NaN and existence > exist_threshold
 *      (exist_threshold = -INFINITY: no existence test).  A non-finite coordinate or NaN existence below c_s sets
 *      WF3D_DECODE_NONFINITE in status[s].
 *   2. greedy suppression: the alive slots visited by (existence descending, slot ascending), floats as values; a slot
 *      within the radius of an earlier representative, d2 <= merge_radius^2 with d2 = (dx dx + dy dy) + dz dz in fp64 (no
 *      FMA), is merged into the first such one in visiting order, else it is a representative.  merge_radius < 0: no
 *      merging; 0: coincident slots only.  A merged slot keeps its representative's coordinates, unchanged.
 *   3. candidate e = (i < j < c_s), e < max_e, survives iff both ends are alive, probs[s, e] > edge_threshold (NaN and
 *      equality do not pass) and the two representatives differ; a pair of representatives takes the maximum probability
 *      of the candidates that land on it (0.0 above -0.0).
 *   4. output vertices = the representatives in slot order (drop_isolated: only the ends of an output edge).
 * Outputs: nverts [B]; dverts [B, V, 3], rows at and past nverts[s] zero; slots [B, V] = the source slot of each output
 * vertex, -1 behind them; koff [B + 1], pairs / seg / kprob (B * max_e rows, the first K = koff[B] packed, the rest left
 * untouched) in the layout of wf3d_edge_compact: pairs in the NEW vertex indices, lexicographic within a sample, end
 * points higher z first (equal z: the second vertex first), so wf3d_hausdorff_lines_batch takes them as they are, and every
 * end point is a row of dverts, as wf3d_eval_metrics_nv requires; status [B].
 * Four launches: one workgroup per sample (slot state in LDS, at most V suppression rounds of one barrier, the per-pair
 * maximum by atomic max in ws), then count / scan / place over the pairs of output vertices.  The only reduction is a
 * maximum: the same bits on every run.  Every loop is bounded by V or max_e, whatever the data.
 * ws: wf3d_wireframe_decode_ws_bytes(B, V, max_e) bytes (4 B V^2 + the chunk counts; 0 when V < 2 or max_e = 0), else
 * WF3D_ERR_WS.  A NaN threshold or radius: WF3D_ERR_ARG.  V <= 1024, B <= 65535, B * max_e < 2^31, else
 * WF3D_ERR_UNSUPPORTED.  B = 0 launches nothing; V < 2 or max_e = 0 still decodes the vertices and writes koff = 0.
 * ------------------------------------------------------------------------ */
#define WF3D_DECODE_NONFINITE 1
size_t wf3d_wireframe_decode_ws_bytes(int B, int V, int max_e);
int wf3d_wireframe_decode(const float* verts, long sample_stride, long vertex_stride, const float* exist, long exist_stride,
                          const int32_t* counts, const float* probs, int B, int V, int max_e, float exist_threshold,
                          float edge_threshold, double merge_radius, int drop_isolated, int32_t* nverts, float* dverts,
                          int32_t* slots, int32_t* koff, int32_t* pairs, float* seg, float* kprob, int32_t* status,
                          void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------
 * Evaluation metrics on the device (csrc/evalmetrics.hip): what eval/ap_calculator.py's compute_metrics derives from a
 * sample's Hausdorff matrix — two rectangular assignments, the corner sets, the counters and the corner distance sum —
 * for a whole batch in four launches.
 *
 * wf3d_lsa_rect_batch: B rectangular linear sum assignments in one launch, one wave per sample.  Sample s's fp64 cost
 * matrix [n_s, m_s] lies row-major at cost + ooff[s] (the layout wf3d_hausdorff_lines_batch writes), with
 * n_s = noff[s * off_stride + 1] - noff[s * off_stride] and m_s likewise from moff (off_stride 1: prefix arrays such as
 * koff / loff; 2: one (begin, end) pair per sample).  Algorithm, association and tie rule are those of wf3d_loss_assign
 * (tests/lsa_model.py::_augmenting_paths).  The solver's rows are the shorter side: the matrix is read transposed
 * (strided, never copied) iff n_s > m_s, as scipy.optimize.linear_sum_assignment does.  col4row + aoff[s] receives
 * min(n_s, m_s) entries: n_s <= m_s: entry i = the column of row i; n_s > m_s: entry j = the row of column j.  Samples
 * with n_s * m_s = 0 write nothing.  A cost that is NaN, +-inf or beyond +-FLT_MAX is read as +-FLT_MAX (NaN: +FLT_MAX),
 * so the search terminates on any input; the scan count of a search and the augmenting walk are also bounded by the row
 * count.  status[s] (always written): WF3D_EVAL_NONFINITE such a cost was met; WF3D_EVAL_STEPS a bound was hit (the
 * entries are then not an assignment); WF3D_EVAL_RANGE max(n_s, m_s) > max_long or a negative extent (nothing written).
 * The solver state lies in LDS while max(n_s, m_s) <= 1024, else in ws: wf3d_lsa_rect_ws_bytes(B, max_long) bytes
 * (0 when max_long <= 1024).  B <= 65535, else WF3D_ERR_UNSUPPORTED.
 *
 * wf3d_eval_metrics: for every sample the counters of APCalculator._with_edges (n_s > 0 kept edges) or _corners_only
 * (n_s = 0) from the Hausdorff matrices hd / ooff of wf3d_hausdorff_lines_batch, in four launches on `stream`:
 *   1. wf3d_lsa_rect_batch on hd -> assign + aoff[s] (aoff: the caller's exclusive prefix of min(n_s, m_s));
 *   2. one workgroup per sample: ok = matched pairs with hd <= thresh, tp_edges their number; pr_u / gt_u = the distinct
 *      end points of the matched predicted / label segments (value equality on the three floats, -0.0 == 0.0); free_pr /
 *      free_gt = the distinct rows of the V predicted / the label vertices not among them, in lexicographic (x, y, z)
 *      order; dm = ||free_pr_i - free_gt_j|| in fp64 ((dx dx + dy dy) + dz dz, no FMA); e_term = sum_i min_j
 *      ||pr_u_i - gt_u_j|| over pr_u in lexicographic order.  n_s = 0: dm over the V and the label vertices as given;
 *   3. wf3d_lsa_rect_batch on the dm matrices;
 *   4. fok = assigned dm <= thresh; distances[s] = (sum of dm[fok] in row order) + e_term; counters[s, 0..8) =
 *      (tp_corners = |pr_u| + sum fok, V, label vertices, tp_edges, n_s, m_s, status, 0).
 * The end points of seg / lseg must be rows of verts / lverts, as wf3d_edge_compact and a gather of the label vertices
 * make them.  status: the solver bits of both launches, WF3D_EVAL_NONFINITE also for a non-finite vertex, matrix entry
 * or thresh; WF3D_EVAL_NO_MATCH kept edges of which none matched (the host path raises there); WF3D_EVAL_RANGE an
 * assignment entry out of range; WF3D_EVAL_ENDPOINT a matched end point that is no vertex row.  A sample with a
 * non-zero status must be evaluated on the host.
 * lvoff / loff: prefix arrays of the label vertices / segments per sample.  max_long >= every n_s and m_s.
 * ws: wf3d_eval_metrics_ws_bytes(B, V, total_lverts, max_long) bytes, total_lverts = lvoff[B].
 * B <= 65535, V <= 1024, max_lverts (>= every sample's label vertex count) <= 1024, B * V and V * total_lverts below
 * 2^31, else WF3D_ERR_UNSUPPORTED; B = 0 launches nothing.
 *
 * wf3d_eval_metrics_nv: the same with a vertex count per sample, for decoded wireframes (wf3d_wireframe_decode's dverts /
 * nverts): sample s's predicted vertices are the first clamp(nverts[s], 0, V) rows of verts[s], counters[s, 1] reports
 * that number, and the rows behind them are never read.  nverts = NULL means V for every sample: wf3d_eval_metrics is
 * that call.  Strides, workspace layout and wf3d_eval_metrics_ws_bytes are the same.
 * ------------------------------------------------------------------------ */
#define WF3D_EVAL_NONFINITE 1
#define WF3D_EVAL_NO_MATCH 2
#define WF3D_EVAL_STEPS 4
#define WF3D_EVAL_RANGE 8
#define WF3D_EVAL_ENDPOINT 16
size_t wf3d_lsa_rect_ws_bytes(int B, long max_long);
int wf3d_lsa_rect_batch(const double* cost, const int64_t* ooff, const int32_t* noff, const int32_t* moff, int off_stride,
                        const int32_t* aoff, int B, long max_long, int32_t* col4row, int32_t* status, void* ws,
                        size_t ws_bytes, void* stream);
size_t wf3d_eval_metrics_ws_bytes(int B, int V, long total_lverts, long max_long);
int wf3d_eval_metrics(const float* verts, long sample_stride, long vertex_stride, int B, int V, const float* seg,
                      const int32_t* koff, const float* lverts, const int32_t* lvoff, const float* lseg, const int32_t* loff,
                      const double* hd, const int64_t* ooff, const int32_t* aoff, int32_t* assign, double thresh,
                      int max_lverts, long total_lverts, long max_long, int32_t* counters, double* distances, void* ws,
                      size_t ws_bytes, void* stream);
int wf3d_eval_metrics_nv(const float* verts, long sample_stride, long vertex_stride, int B, int V, const int32_t* nverts,
                         const float* seg, const int32_t* koff, const float* lverts, const int32_t* lvoff, const float* lseg,
                         const int32_t* loff, const double* hd, const int64_t* ooff, const int32_t* aoff, int32_t* assign,
                         double thresh, int max_lverts, long total_lverts, long max_long, int32_t* counters,
                         double* distances, void* ws, size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* WF3D_H */
