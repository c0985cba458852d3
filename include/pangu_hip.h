/*
 * pangu_hip.h — C ABI of the MI355X (gfx950) kernels behind the Pangu-Weather hot path.
 *
 * Drop-in boundary.  The reference (zhaoshan2/pangu-pytorch) has no native layer: its "operator API" for
 * this path is the nn.Module surface of models/pangu_model.py:8-87 and the layer classes of
 * models/layers.py.  This library sits UNDER that surface: each entry point replaces the ATen-op chain of
 * one reference method (cited per function) and is what a ctypes/cffi binding on the reference side binds
 * (see INTEGRATION.md).  Plain pointers and sizes only — no torch types.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless stated; tensors are dense row-major fp32 (dtype-tagged
 *     variants take PANGU_F32 / PANGU_BF16 where noted);
 *   - `stream` is a hipStream_t passed as void*; nothing allocates, synchronises or branches on device
 *     data on the host => every call is hipGraph-capturable;
 *   - return value: PANGU_OK (0), a negative PANGU_E_* for bad arguments (nothing launched), or a positive
 *     hipError_t if the launch itself failed;
 *   - token tensors are (N, C) with N = Z*H*W tokens in (z,h,w) order (reference layers.py:188,247),
 *     row stride given explicitly as `ld*` (in elements) where a kernel supports strided rows.
 */
#ifndef PANGU_HIP_H
#define PANGU_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PANGU_ABI_VERSION 1

#define PANGU_OK 0
#define PANGU_E_SHAPE (-1)     /* unsupported shape / divisibility */
#define PANGU_E_NULL (-2)      /* required pointer is NULL */
#define PANGU_E_DTYPE (-3)     /* unsupported dtype tag */
#define PANGU_E_ARG (-4)       /* other invalid argument */
#define PANGU_E_RANGE (-5)     /* a row-strided matrix spans 4 GB or more: the linear / wgrad entries use 32-bit byte
                                  offsets (range-checked buffer addressing); split the call by rows */

#define PANGU_F32 0
#define PANGU_BF16 1

#define PANGU_ACT_NONE 0
#define PANGU_ACT_GELU 1       /* exact erf GELU, reference layers.py:261; aux (optional) receives the pre-activation */
#define PANGU_ACT_GELU_BWD 2   /* C = (A @ W^T) * gelu'(aux): backward through the GELU, aux = saved pre-activation */
#define PANGU_ACT_ADD 3        /* C = A @ W^T + bias + aux: residual-gradient accumulation fused into the data-gradient GEMM */
#define PANGU_ACT_GELU_BWD_H 4 /* bf16 only (pangu_linear_gelu_bwd_bf16): PANGU_ACT_GELU_BWD, and h = GELU(aux) is written too */

typedef void* pangu_stream_t;  /* hipStream_t */

int pangu_abi_version(void);
const char* pangu_error_string(int code);

/* ---- integer contract (bit-exact vs oracle) ------------------------------------------------------- */

/* out[nLon][types][144] int32: source token of every window slot, -1 = zero pad.
 * Replaces view/pad/roll/partition of EarthSpecificBlock.forward, reference layers.py:188-221. */
int pangu_window_index_export(pangu_stream_t stream, int32_t* out, int Z, int H, int W, int shifted);

/* out[types][144][144] fp32 in {0,-100}: shifted-window mask, reference layers.py:153-181 (gen_mask). */
int pangu_window_mask_export(pangu_stream_t stream, float* out, int Z, int H, int W);

/* ---- dense projections ---------------------------------------------------------------------------- */

/* C[M,N] = act(A[M,K] @ W[N,K]^T + bias[N]).  W is the torch nn.Linear / Conv1d(k=1) weight as stored
 * (out,in).  bias may be NULL.  K % 16 == 0, N % 4 == 0.  aux [M][N] (dense): see PANGU_ACT_*; NULL otherwise.
 * Replaces nn.Linear / nn.Conv1d calls at reference layers.py:68,86,265-268,365,418,457,476,498,520,536.
 * The input-gradient of a projection is the same call with W^T: dA[M,K] = dC[M,N] @ (W^T)[K,N]^T. */
int pangu_linear_fwd(pangu_stream_t stream, const float* A, int lda, const float* W, const float* bias,
                     float* C, int ldc, int M, int N, int K, int act, float* aux);

/* The same product for frozen fp32 inference on the bf16 matrix pipe, bit-for-bit fp32 operands: every fp32 value is the exact
 * sum of three bf16 values (hi, mid, lo), and the six partial products of order >= 2^-16 are accumulated in fp32 (error at the
 * level of pangu_linear_fwd's own: profiles/f32_split_error.md).
 * Both serve N > 0, N % 4 == 0, K % 16 == 0; PANGU_E_SHAPE otherwise means "not served": call pangu_linear_fwd.
 *   pangu_split_weight_bf16x3: W[N,K] fp32 -> `image`, 6 * rows * K bytes, rows = 192 * ceil(N / 192): the three bf16 planes in
 *     the fragment order of the GEMM, [rows/192][K/16][plane][k-half][192 rows][8 bf16]; the rows >= N are zero rows (+0 in
 *     all three planes, never read from W).  Once per weight.
 *   pangu_linear_fwd_split: C = act(A @ W^T + bias) from that image; A / C row-strided fp32, any M, act NONE or GELU.  It runs
 *     whole 192-column tiles over the image; where N % 192 != 0 a column guard keeps it from reading bias[N..] and from writing
 *     a column >= N of C (ldc may exceed N): per element the product on the zero-extended weight, bit for bit. */
int pangu_split_weight_bf16x3(pangu_stream_t stream, const float* W, int N, int K, void* image);
int pangu_linear_fwd_split(pangu_stream_t stream, const float* A, int lda, const void* image, const float* bias,
                           float* C, int ldc, int M, int N, int K, int act);

/* Weight/bias gradient of a projection (autograd of the calls above; the training step of reference
 * models/pangu_sample.py:71 `loss.backward()`):
 *   dW[N,K] += dC[M,N]^T @ A[M,K]      db[N] += sum_m dC[m,:]   (db may be NULL)
 * ACCUMULATES with fp32 atomics into caller-initialised buffers (zero them, or pass live .grad buffers). */
int pangu_linear_wgrad(pangu_stream_t stream, const float* dC, int lddc, const float* A, int lda, float* dW,
                       float* db, int M, int N, int K);
/* The same product with a caller-owned scratch buffer (see pangu_linear_wgrad_bf16_ws): partial tiles of the token slabs
 * through the buffer + one reduce launch instead of fp32 atomics; NULL / too small = the entry above. */
int pangu_linear_wgrad_ws(pangu_stream_t stream, const float* dC, int lddc, const float* A, int lda, float* dW,
                          float* db, int M, int N, int K, float* workspace, long long workspace_bytes);

/* ---- LoRA adapters (peft's lora.Linear on a frozen projection: reference finetune/lora_tune.py:124-135) --------------- */

/* Adapter gradients of y = X W_eff^T + b, W_eff = W + s * B A, A [r][K], B [N][r], s = alpha / r:
 *   dA[r][K] = s * (dY B)^T X        dB[N][r] = s * dY^T (X A^T)
 * ONE pass over X [M][K] (row stride ldx) and dY [M][N] (row stride lddy); WRITES dA / dB (no accumulation).  Per-workgroup
 * partials go through `workspace` (>= r*(K+N)*4 bytes, 16-B aligned; more lets more workgroups run) and one reduce launch:
 * deterministic, no atomics.  r in {4, 8, 16, 32}; K, N multiples of 16 with K + N <= 1920; X, dY, A 16-B aligned. */
int pangu_lora_wgrad_f32(pangu_stream_t stream, const float* dY, int lddy, const float* X, int ldx, const float* A,
                         const float* B, float* dA, float* dB, int M, int N, int K, int r, float scaling, float* workspace,
                         long long workspace_bytes);
/* The same gradients on the bf16 training path: X and dY are bf16 (row strides in elements, multiples of 8), A and B the fp32
 * master parameters, rounded to nearest-even bf16 by the kernel; every product is bf16 MFMA with fp32 accumulation, U = X A^T and
 * V = dY B are rounded to bf16 once; dA / dB are fp32, WRITTEN, scaled in fp32.  Same workspace / determinism contract and error
 * codes as the fp32 entry; X, dY, A, B and the workspace 16-B aligned. */
int pangu_lora_wgrad_bf16(pangu_stream_t stream, const void* dY, int lddy, const void* X, int ldx, const float* A, const float* B,
                          float* dA, float* dB, int M, int N, int K, int r, float scaling, float* workspace,
                          long long workspace_bytes);
/* W_eff[N][K] = W + s * (B A), the rank sum in the fixed order 0..r-1 (dense fp32; r in {4, 8, 16, 32}); capturable. */
int pangu_lora_merge_f32(pangu_stream_t stream, const float* W, const float* A, const float* B, float* W_eff, int N, int K,
                         int r, float scaling);

/* ---- LoRA adapter dropout (peft's lora_dropout; fp32).  In training mode peft computes y = X W^T + b + s * drop(X) A^T B^T with
 * drop(X) = keep * X / (1 - p).  The projection kernels run on W_eff, so with c = keep / (1 - p) - 1 the dropout is an additive
 * correction after the projection's forward launch and after its input-gradient GEMM.  The keep mask is a pure function of
 * (seed, row i of the [M][K] operand, column k) and is never stored:
 *   keep(seed, i, k) = lowbias32(lowbias32(lowbias32(seed) ^ i) ^ k) >= T,   T = clamp(floor(p * 2^32 + 0.5), 1, 2^32 - 1),
 *   lowbias32(x): x ^= x>>16; x *= 0x7feb352d; x ^= x>>15; x *= 0x846ca68b; x ^= x>>16   (uint32).
 * Common contract: 0 < p < 1 (PANGU_E_ARG otherwise), r in {4, 8, 16, 32}, K and N multiples of 64 with K + N <= 1920, row strides
 * multiples of 4 floats, every pointer 16-B aligned; no atomics, bit-identical from run to run; capturable. */

/* Y[M][N] (row stride ldy) += s * ((c * X) A^T) B^T, in place, X [M][K] (row stride ldx).  act = PANGU_ACT_GELU: H[M][N] (row
 * stride ldh) = gelu(Y) of the corrected Y is written as well (the MLP's first projection then runs its GEMM without the GELU
 * epilogue); PANGU_ACT_NONE: H is not touched (may be NULL). */
int pangu_lora_dropout_fwd_f32(pangu_stream_t stream, const float* X, int ldx, float* Y, int ldy, const float* A, const float* B,
                               int M, int N, int K, int r, float scaling, double p, unsigned seed, int act, float* H, int ldh);
/* pangu_lora_wgrad_f32 with drop(X) in place of X: dA = s * (dY B)^T drop(X), dB = s * dY^T (drop(X) A^T), and one more output,
 * V[M][r] = s * dY B (dense), which pangu_lora_dropout_dx_f32 reads.  Workspace and error codes as pangu_lora_wgrad_f32. */
int pangu_lora_wgrad_dropout_f32(pangu_stream_t stream, const float* dY, int lddy, const float* X, int ldx, const float* A,
                                 const float* B, float* dA, float* dB, float* V, int M, int N, int K, int r, float scaling, double p,
                                 unsigned seed, float* workspace, long long workspace_bytes);
/* dX[M][K] (row stride lddx) += c * (V A), in place, V [M][r] from the entry above.  pre (optional, [M][K], row stride ldpre):
 * the projection's input is gelu(pre) and dX already holds the gradient of pre (PANGU_ACT_GELU_BWD epilogue of the dX GEMM); the
 * correction is multiplied by gelu'(pre) as well. */
int pangu_lora_dropout_dx_f32(pangu_stream_t stream, float* dX, int lddx, const float* V, const float* A, int M, int K, int r,
                              double p, unsigned seed, const float* pre, int ldpre);

/* ---- LoRA adapter dropout on the bf16 training path.  The arithmetic and the mask are those of the fp32 entries above (the same
 * keep(seed, i, k), recomputed in every kernel, never stored; p is a double so that host and device form the same T), on bf16
 * activations.  Common contract: 0 < p < 1 (PANGU_E_ARG otherwise), r in {4, 8, 16, 32}, K and N multiples of 64 with K + N <= 1920;
 * bf16 operands are row-strided with strides in elements that are multiples of 8 and at least the row; every pointer 16-B aligned.
 * A [r][K] and B [N][r] are the fp32 master adapters, rounded to nearest-even bf16 by the kernel (as pangu_lora_wgrad_bf16 does);
 * products are bf16 MFMA with fp32 accumulation.  No atomics, bit-identical from run to run; capturable.  Arguments are checked
 * before any memory is touched, with the error codes of pangu_lora_wgrad_bf16: PANGU_E_NULL (a required pointer), PANGU_E_SHAPE (M,
 * r, K, N, a stride), PANGU_E_ARG (alignment, p, act, a workspace that is too small). */

/* In place on the bf16 Y[M][N] (row stride ldy): v = float(Y) + s * ((c * X) A^T) B^T in fp32, Y = bf16(v); X [M][K] bf16 (row
 * stride ldx).  c * X and u = s (c * X) A^T are rounded to bf16 once each.  act = PANGU_ACT_GELU: H[M][N] (row stride ldh) =
 * bf16(gelu(float(bf16(v)))), the exact-erf GELU of the ROUNDED value -- what pangu_linear_gelu_bwd_bf16 re-creates from the stored
 * Y in the backward; PANGU_ACT_NONE: H is not touched (may be NULL). */
int pangu_lora_dropout_fwd_bf16(pangu_stream_t stream, const void* X, int ldx, void* Y, int ldy, const float* A, const float* B,
                                int M, int N, int K, int r, float scaling, double p, unsigned seed, int act, void* H, int ldh);
/* pangu_lora_wgrad_bf16 with drop(X) in place of X: dA = s * (dY B)^T drop(X), dB = s * dY^T (drop(X) A^T), and one more output,
 * V[M][r] = s * dY bf16(B) (dense fp32, from the fp32 partials before their bf16 rounding), which pangu_lora_dropout_dx_bf16
 * reads.  The mask is applied exactly (dropped entries zeroed, 1 / (1 - p) applied in fp32 with s): dropout adds no rounding to
 * dA / dB.  Workspace and error codes as pangu_lora_wgrad_bf16. */
int pangu_lora_wgrad_dropout_bf16(pangu_stream_t stream, const void* dY, int lddy, const void* X, int ldx, const float* A,
                                  const float* B, float* dA, float* dB, float* V, int M, int N, int K, int r, float scaling, double p,
                                  unsigned seed, float* workspace, long long workspace_bytes);
/* In place on the bf16 dX[M][K] (row stride lddx): dX = bf16(float(dX) + c * (V A) [* gelu'(float(pre))]), V [M][r] fp32 from the
 * entry above (rounded to bf16 once).  pre: optional bf16 [M][K] (row stride ldpre), as in pangu_lora_dropout_dx_f32. */
int pangu_lora_dropout_dx_bf16(pangu_stream_t stream, void* dX, int lddx, const float* V, const float* A, int M, int K, int r,
                               double p, unsigned seed, const void* pre, int ldpre);

/* ---- Earth-specific window attention -------------------------------------------------------------- */

/* Fused roll + window partition + (q*scale)k^T + earth_specific_bias + shift mask + softmax + .v +
 * window reverse + roll back + crop, one (window, head) per workgroup.
 *   qkv  [N][3C]  linear1 output on the UNPADDED tokens (channel = which*C + head*32 + d, layers.py:368-371)
 *   qkv_bias [3C] linear1.bias: the q/k/v of zero-pad tokens (layers.py:192 pads before linear1)
 *   esb  [types][heads][144][144] earth_specific_bias (layers.py:306-311)
 *   out  [N][C]   attention output before linear2 (channel = head*32 + d, layers.py:413-415)
 *   lse  [N][heads] optional (may be NULL): log-sum-exp of each query row, saved for backward
 * Replaces reference layers.py:192-247 + :368-415. */
int pangu_window_attn_fwd(pangu_stream_t stream, const float* qkv, const float* qkv_bias, const float* esb,
                          float* out, float* lse, int Z, int H, int W, int C, int heads, int shifted);
/* Inference mode on the paper's COMPACT Earth-specific bias: esb_compact is [types][heads][3312] fp32 (the (3312, types, heads)
 * table of reference layers.py:306-357 with the index axis last); the kernel gathers each score's bias through the
 * position index in closed form (layers.py:319-357, :384-391) -- 13 KB per (type, head) instead of 83 KB, 10 MB instead
 * of 62 MB per block.  Bit-identical to pangu_window_attn_fwd on the expanded table of the same values. */
int pangu_window_attn_fwd_compact(pangu_stream_t stream, const float* qkv, const float* qkv_bias,
                                  const float* esb_compact, float* out, float* lse, int Z, int H, int W, int C,
                                  int heads, int shifted);
/* The same two forwards for frozen INFERENCE with both contractions computed as exact-split bf16 MFMA products (each fp32 operand
 * the exact sum of three bf16 values, six products per term into one fp32 accumulator: csrc/attn_f32_split.hip); error at the
 * level of the fp32-MFMA kernel's own.  No lse is produced: training keeps pangu_window_attn_fwd.  The two bias modes are
 * bit-identical to each other. */
int pangu_window_attn_fwd_split(pangu_stream_t stream, const float* qkv, const float* qkv_bias, const float* esb,
                                float* out, int Z, int H, int W, int C, int heads, int shifted);
int pangu_window_attn_fwd_split_compact(pangu_stream_t stream, const float* qkv, const float* qkv_bias,
                                        const float* esb_compact, float* out, int Z, int H, int W, int C, int heads,
                                        int shifted);

/* EarthAttention3D.forward's own calling convention (reference layers.py:360-421, the part between linear1 and linear2) for
 * callers that use the module OUTSIDE EarthSpecificBlock: the tensor is already partitioned and the mask is explicit.
 *   qkv  [n_lon*types*144][3C]  linear1 output of the window slots in (lon window, type, slot) order (every slot an ordinary
 *                               token: nothing is a pad here), channel = which*C + head*32 + d
 *   esb  [types][heads][144][144]
 *   mask NULL (layers.py:404-405) or fp32 [n_lon][types][144][144] with mask_lon_stride = types*144*144, or one
 *        [types][144][144] table shared by all longitude windows with mask_lon_stride = 0 (layers.py:401-402)
 *   out  [n_lon*types*144][C]   channel = head*32 + d (layers.py:413-415)
 * Not on the hot path (plain VALU kernel, one (window, head) per workgroup). */
int pangu_attn_windows_fwd(pangu_stream_t stream, const float* qkv, const float* esb, const float* mask,
                           long long mask_lon_stride, float* out, int n_lon, int types, int heads, int C);

/* Backward of pangu_attn_windows_fwd: dout [rows][C] -> dqkv [rows][3C] (every row written), d_esb [types][heads][144][144]
 * (overwritten: summed over the n_lon windows inside the kernel, no atomics).  The mask gets no gradient (layers.py:153-181 builds
 * it from constants). */
int pangu_attn_windows_bwd(pangu_stream_t stream, const float* qkv, const float* esb, const float* mask,
                           long long mask_lon_stride, const float* dout, float* dqkv, float* d_esb, int n_lon, int types,
                           int heads, int C);

/* Backward of pangu_window_attn_fwd.  One workgroup per (window type, head) walks the nLon longitude windows
 * and keeps the bias gradient d_esb[t][head] = sum_l dS in registers (no atomics, written once).
 *   out, lse: the forward's outputs;  dout [N][C]: gradient w.r.t. out
 *   dqkv [N][3C]: gradient w.r.t. qkv (every real token is written exactly once per q/k/v)
 *   dqkv_bias [3C]: ACCUMULATED (atomics) gradient reaching linear1.bias through the zero-pad slots
 *   d_esb [types][heads][144][144]: overwritten */
int pangu_window_attn_bwd(pangu_stream_t stream, const float* qkv, const float* qkv_bias, const float* esb,
                          const float* out, const float* lse, const float* dout, float* dqkv, float* dqkv_bias,
                          float* d_esb, int Z, int H, int W, int C, int heads, int shifted);

/* ---- row kernels ----------------------------------------------------------------------------------- */

/* out[r] = shortcut[r] + branch_scale * (LayerNorm(y[r]) * gamma + beta)
 * (post-norm residual, reference layers.py:250-251; branch_scale = 1 in eval, the DropPath keep factor
 * 1/(1-p) in training, timm DropPath semantics).  eps = 1e-5.  shortcut/out may have row strides != C
 * (lds/ldo).  mean_rstd (may be NULL): [N][2] saved statistics for backward. */
int pangu_ln_residual_fwd(pangu_stream_t stream, const float* y, const float* shortcut, int lds,
                          const float* gamma, const float* beta, float* out, int ldo, float* mean_rstd,
                          int N, int C, float branch_scale);

/* Projection + post-norm residual in one launch (inference path of layers.py:250-251), fp32, N = 192 only (the GEMM tile
 * spans the whole row):  out[M,N] = shortcut[M,N] + branch_scale * (LayerNorm(A[M,K] @ W[N,K]^T + bias) * gamma + beta).
 * shortcut / out row strides lds / ldo; bias may be NULL; K % 16 == 0.  Replaces pangu_linear_fwd + pangu_ln_residual_fwd. */
int pangu_linear_ln_residual_fwd(pangu_stream_t stream, const float* A, int lda, const float* W, const float* bias,
                                 const float* shortcut, int lds, const float* gamma, const float* beta, float* out, int ldo,
                                 int M, int N, int K, float branch_scale);

/* The same fused op for frozen fp32 inference with the product on the bf16 matrix pipe: W given as its exact-split image
 * (pangu_split_weight_bf16x3: for N = 384 the kernel reads the image's two 192-row n-tile blocks of every k-step), six partial
 * products into one fp32 accumulator as in pangu_linear_fwd_split, the LayerNorm / residual epilogue of
 * pangu_linear_ln_residual_fwd operation for operation (error: profiles/f32_split_ln_error.md).  Same arguments otherwise, same
 * checks and error codes: N = 192 or 384, K % 16 == 0, bias may be NULL. */
int pangu_linear_ln_residual_fwd_split(pangu_stream_t stream, const float* A, int lda, const void* image, const float* bias,
                                       const float* shortcut, int lds, const float* gamma, const float* beta, float* out,
                                       int ldo, int M, int N, int K, float branch_scale);

/* Backward of the LayerNorm branch of pangu_ln_residual_fwd (the shortcut's gradient is dout itself):
 *   dy [N][C] overwritten;  dgamma[C], dbeta[C] ACCUMULATED (atomics).  dout may be row-strided (lddo). */
int pangu_ln_residual_bwd(pangu_stream_t stream, const float* dout, int lddo, const float* y, const float* gamma,
                          float* dy, float* dgamma, float* dbeta, int N, int C, float branch_scale);

/* DownSample gather + LayerNorm(4C): x[Z][H][W][C] (row stride ldx) -> out[Z*(H+1)/2*(W/2)][4C],
 * channel = dh*2C + dw*C + c, zero row for h == H (pad).  Reference layers.py:436-454. */
int pangu_downsample_ln_fwd(pangu_stream_t stream, const float* x, int ldx, const float* gamma,
                            const float* beta, float* out, float* mean_rstd, int Z, int H, int W, int C);

/* Backward: dout [rows][4C] -> dx [Z*H*W][C] (overwritten, every token once); dgamma/dbeta [4C] ACCUMULATED.
 * dx_add (may be NULL): a second gradient of the same tokens, dense [Z*H*W][C] -- the skip connection's (reference
 * pangu_model.py:62,81: layer 0's output feeds both the down-sampling and the channel concat) -- added to dx in this pass
 * instead of by a separate elementwise kernel. */
int pangu_downsample_ln_bwd(pangu_stream_t stream, const float* dout, const float* x, int ldx, const float* gamma,
                            float* dx, float* dgamma, float* dbeta, int Z, int H, int W, int C, const float* dx_add);

/* UpSample pixel-shuffle + crop + LayerNorm(Co): y[Z][H2][W2][4*Co] -> out[Z][H][2*W2][Co] with
 * out[z][2h+dh][2w+dw][c] = y[z][h][w][dh*2Co + dw*Co + c], rows h >= H dropped.  Reference layers.py:480-495.
 * pre (may be NULL): the shuffled rows before LayerNorm, saved for backward. */
int pangu_upsample_ln_fwd(pangu_stream_t stream, const float* y, const float* gamma, const float* beta,
                          float* out, float* mean_rstd, int Z, int H2, int W2, int H, int Co);

/* Backward: dout [Z*H*2W2][Co] -> dy [Z*H2*W2][4Co] (overwritten; cropped rows get 0); dgamma/dbeta ACCUMULATED. */
int pangu_upsample_ln_bwd(pangu_stream_t stream, const float* dout, const float* y, const float* gamma, float* dy,
                          float* dgamma, float* dbeta, int Z, int H2, int W2, int H, int Co);

/* ---- patch embedding / recovery --------------------------------------------------------------------- */

/* Normalise + zero-pad + patchify the raw fields into GEMM A-matrices (reference layers.py:48-85):
 *   a_surface [H4*W4][112]  col = c*16 + ph*4 + pw,  c<4: (input_surface-mean)/std, c in 4..6: maps
 *   a_upper [7*H4*W4][192]  col = c*32 + pz*16 + ph*4 + pw, c<5: (input-mean_used)/std_used, c==5: const_h
 * with mean_used[c][l] = upper_mean[12-l][c] (level-reversed statistics, layers.py:73-76).
 * input [5][13][LAT][LON], input_surface [4][LAT][LON], maps [3][4*H4][LON], const_h [13][LAT][LON],
 * surface_mean/std [4], upper_mean/std [13][5].  LAT=721, LON=1440 -> H4=181, W4=360.
 * levels_reversed != 0: `input` is stored with its level axis in the file's (ascending) order and the reader's reversal
 * (reference era5_data/utils_data.py:117, `[::-1]` on the host) is done by this kernel's addressing: logical level l is read
 * from plane 12 - l.  Statistics, const_h and the outputs are unaffected. */
int pangu_patch_embed_gather(pangu_stream_t stream, const float* input, const float* input_surface,
                             const float* surface_mean, const float* surface_std, const float* upper_mean,
                             const float* upper_std, const float* maps, const float* const_h,
                             float* a_surface, float* a_upper, int LAT, int LON, int levels_reversed);

/* Adjoint of the gather above w.r.t. the raw fields (autograd of reference layers.py:48-55,71-76 when a caller sets
 * input.requires_grad): d_input [5][13][LAT][LON] = da_upper[token][c*32+pz*16+ph*4+pw] / upper_std[12-l][c],
 * d_input_surface [4][LAT][LON] = da_surface[token][c*16+ph*4+pw] / surface_std[c]; every element of both fields is
 * written.  da_surface [H4*W4][64], da_upper [7*H4*W4][160] fp32: the gradient of the A-matrices' field columns only (the
 * first 64 of 112 / 160 of 192; the columns of maps / const_h have no field behind them).
 * levels_reversed as in the forward: d_input is laid out like the `input` it belongs to. */
int pangu_patch_embed_gather_bwd(pangu_stream_t stream, const float* da_surface, const float* da_upper,
                                 const float* surface_std, const float* upper_std, float* d_input,
                                 float* d_input_surface, int LAT, int LON, int levels_reversed);

/* Un-patchify + crop (reference layers.py:522-543):
 *   y_upper [7*H4*W4][160] col = v*32 + pz*16 + ph*4 + pw -> output [5][13][LAT][LON]
 *   y_surface [H4*W4][64]  col = v*16 + ph*4 + pw          -> output_surface [4][LAT][LON] */
int pangu_patch_recover_scatter(pangu_stream_t stream, const float* y_upper, const float* y_surface,
                                float* output, float* output_surface, int LAT, int LON);
/* The same scatter with the reference's `normBackData` (era5_data/utils_data.py:324-330) folded in for the rollout: besides
 * the normalised fields every element is also written in physical units, phys = out * std + mean (a multiply, then an add,
 * as the reference's expression rounds) of its (variable, level) plane, into phys [5][13][LAT][LON] / phys_surface
 * [4][LAT][LON] -- the next step's input buffers.  upper_mean / upper_std: [5][13] (the `weather_statistics_last` layout,
 * utils_data.py:214-236), surface_mean / surface_std: [4]. */
int pangu_patch_recover_scatter_denorm(pangu_stream_t stream, const float* y_upper, const float* y_surface, float* output,
                                       float* output_surface, float* phys, float* phys_surface, const float* upper_mean,
                                       const float* upper_std, const float* surface_mean, const float* surface_std, int LAT,
                                       int LON);

/* Backward of the scatter: gradients of the two field tensors -> dy_upper [7*H4*W4][160], dy_surface [H4*W4][64]
 * (cropped positions get 0). */
int pangu_patch_recover_gather_bwd(pangu_stream_t stream, const float* d_output, const float* d_output_surface,
                                   float* dy_upper, float* dy_surface, int LAT, int LON);

/* ---- evaluation ---------------------------------------------------------------------------- */

/* Latitude-weighted sums behind RMSE / ACC (reference era5_data/score.py:92-105,123-135), per plane of pred/target
 * [planes][H][W]:  out[plane] = { sum w (p-t)^2, sum w p t, sum w p^2, sum w t^2 } with lat_weight w[H].
 * ACCUMULATES (atomics) into a zero-initialised out[planes][4].  W % 4 == 0. */
int pangu_lat_weighted_sums(pangu_stream_t stream, const float* pred, const float* target, const float* lat_weight,
                            float* out, int planes, int H, int W);

/* ---- ensembles (Pangu-Weather paper: initial states perturbed with Perlin noise) ------------------------------------- */

/* Adds amplitude[var] * std[plane] * noise, in place, to E member states upper [E][5][13][H][W] and surface [E][4][H][W]
 * (member strides in elements, multiples of 4; upper / surface 16-B aligned).  noise = sum_{o < octaves} persistence^o *
 * perlin_o, 2-D Perlin gradient noise with period * 2^o lattice cells around the longitude circle (W % that == 0, wrapping at
 * the dateline; the octaves' lattice columns plus one each sum to at most 1024; octaves 1..8).  Plane p = var*13 + level
 * (upper), 65 + var (surface); amplitude [9], upper_std [65], surface_std [4] are device arrays.  Member e is global member
 * first_member + e: its noise depends on (seed, member, plane, position) alone.  control != 0 leaves member 0 untouched.
 * The definition is pinned in csrc/ensemble.hip.  W % 4 == 0. */
int pangu_ensemble_perturb_f32(pangu_stream_t stream, float* upper, long long upper_member_stride, float* surface,
                               long long surface_member_stride, int E, int first_member, int H, int W, const float* amplitude,
                               const float* upper_std, const float* surface_std, unsigned int seed, int octaves, int period,
                               float persistence, int control);

/* Latitude-weighted ensemble scores per plane of members [E][planes][H][W] (member stride in elements), 2 <= E <= 128, W % 4 == 0:
 *   out[plane] = { rmse_mean = sqrt(sum w (m-y)^2 / N), acc_mean = sum w (m-c)(y-c) / sqrt(sum w (m-c)^2 sum w (y-c)^2),
 *                  spread = sqrt(sum w var / N), crps = sum w crps_fair / N }
 * with N = H*W, lat_weight w [H], m the ensemble mean, var the unbiased member variance, c = clim[plane] and
 * crps_fair = (1/E) sum_i |x_i - y| - 1/(2E(E-1)) sum_i sum_j |x_i - x_j|.  target y [planes][H][W] may be NULL (then only
 * spread is computed, the rest is NaN; clim may be NULL too).  mean_out / std_out [planes][H][W] (may be NULL) receive the
 * mean and the square root of var.  Per-workgroup partials go through workspace (>= planes * ceil(H / 4) * 32 bytes) and one
 * fixed-order reduce launch: deterministic, no atomics.  out 16-B aligned. */
int pangu_ensemble_stats_f32(pangu_stream_t stream, const float* members, long long member_stride, int E, const float* target,
                             const float* clim, const float* lat_weight, float* out, float* mean_out, float* std_out,
                             float* workspace, long long workspace_bytes, int planes, int H, int W);

/* Ensemble reliability of members [E][planes][H][W] (member stride in elements, a multiple of 4), 2 <= E <= 128, 0 <= T <= 4,
 * W % 4 == 0, in one streaming pass (csrc/reliability.hip pins the definitions).  Per grid point of plane p:
 *   rank = #{x_i < y} + floor(u * (#{x_i == y} + 1) / 2^32), u a hash of (seed, first_plane + p, h*W + w): ties broken uniformly;
 *   k_t  = #{x_i > thresholds[t][p]} (strict), o_t = (y > thresholds[t][p]).
 * counts [planes][1 + 2T][E + 1] (uint32): table 0 the verification rank histogram, table 1 + 2t the number of points N_t per
 * k_t, table 2 + 2t the number of those with the event observed, O_t.  freq, same shape: each point weighted by lat_weight[h]
 * (H values) and divided by H*W.  prob [T][planes][H][W] (may be NULL; must be NULL with T == 0) receives k_t / E.  target y
 * [planes][H][W] may be NULL (forecast mode; needs T > 0): table 0 and every O_t are then zero.  thresholds [T][planes] in the
 * members' units (NULL iff T == 0); +inf is an event that never happens.  Non-finite values are NOT detected: a comparison with
 * NaN is false.  workspace >= planes * ceil(H / 4) * (1 + 2T) * (E + 1) * 8 bytes.  Integer counts through per-slab partials
 * and one fixed-order reduce launch, no floating-point atomics: counts are exact, freq is bit-identical from run to run.
 * PANGU_E_NULL: a required pointer, prob with T == 0, or neither target nor thresholds; PANGU_E_SHAPE: E, T, W % 4, first_plane < 0,
 * a non-positive size, H*W >= 2^31, a member stride that is short or no multiple of 4, (E - 1) * stride + planes*H*W > 2^40;
 * PANGU_E_ARG: a workspace that is too small, or members / target / counts / freq / prob / workspace not 16-B aligned. */
int pangu_ensemble_reliability_f32(pangu_stream_t stream, const float* members, long long member_stride, int E,
                                   const float* target, const float* thresholds, int T, const float* lat_weight,
                                   unsigned int seed, int first_plane, unsigned int* counts, float* freq, float* prob,
                                   void* workspace, long long workspace_bytes, int planes, int H, int W);

/* Ensemble quantile fields and quantile scores of members [E][planes][H][W] (member stride in elements), 2 <= E <= 128,
 * 1 <= Q <= 8 levels, W % 4 == 0, in one streaming pass (csrc/quantile.hip pins the definitions).  levels: Q HOST doubles in
 * [0, 1].  Per level, in double: h = q * (E - 1), lo = floor(h), frac = (float)(h - lo).  Per grid point, with x_(0) <= ... <=
 * x_(E-1) the RAW member values sorted:
 *   frac == 0:  x_(lo), a pure selection (q = 0, q = 1, the median of an odd E: a member's bits, also beside +-inf members);
 *   otherwise:  fmin(fmax(fmaf(frac, x_(lo+1) - x_(lo), x_(lo)), x_(lo)), x_(lo+1)): numpy's "linear" method clamped into its
 *               bracket, so the fields are monotone in q at every point.
 * A point where any member is NaN gets NaN in every field, contributes nothing to the scores and counts, and is counted in
 * nonfinite [planes] (uint32, required).  fields [Q][planes][H][W] may be NULL when only scores are wanted.  With target y
 * [planes][H][W] (then lat_weight [H], pinball, coverage_count and coverage_freq are required; all three [Q][planes]):
 *   pinball        = sum w_h rho_q(y - x_q) / (H*W),  rho_q(u) = u * (q - (u < 0 ? 1 : 0))   (integrates over q to CRPS / 2);
 *   coverage_count = #{points : y <= x_q} (uint32), against the very fp32 value written to fields;
 *   coverage_freq  = the same points weighted by lat_weight[h], divided by H*W (near q for a calibrated ensemble).
 * Without a target the three score outputs are not written (they may be NULL) and fields is required.  workspace >=
 * pangu_ensemble_quantiles_ws_bytes(planes, H, Q) = planes * ceil(H / 4) * (3Q + 1) * 4 bytes (host-only; PANGU_E_SHAPE for sizes
 * out of range), 4-B aligned.  Per-slab partials and one fixed-order reduce launch (slabs added in double), no atomics: every
 * output is bit-identical from run to run.  Two launches on `stream`, no host sync; everything is checked before the first.
 * PANGU_E_NULL: a required pointer, or neither fields nor target; PANGU_E_SHAPE: E, Q, W % 4, a non-positive size, H*W >= 2^31,
 * W >= 2^22, a short member stride, (E - 1) * stride + planes*H*W or Q*planes*H*W > 2^40; PANGU_E_ARG: a level outside [0, 1] or
 * NaN, a workspace that is too small or misaligned. */
long long pangu_ensemble_quantiles_ws_bytes(int planes, int H, int Q);
int pangu_ensemble_quantiles_f32(pangu_stream_t stream, const float* members, long long member_stride, int E,
                                 const double* levels, int Q, const float* target, const float* lat_weight, float* fields,
                                 float* pinball, unsigned int* coverage_count, float* coverage_freq, unsigned int* nonfinite,
                                 void* workspace, long long workspace_bytes, int planes, int H, int W);

/* Zonal power spectra of fields [N][planes][H][W] (item stride in elements, a multiple of 4), averaged over 1 <= B <= 4 latitude
 * bands band_weight [B][H], for the wavenumbers 0..K, 1 <= K <= W/2; W % 4 == 0, W >= 8 (csrc/spectrum.hip pins the definitions).
 * Per row, in fp32: d = fields - minus (one rounding; minus [planes][H][W] may be NULL: d = fields), pivot = d[0], a = d - pivot
 * (a constant changes only wavenumber 0; the pivot takes the large offset of geopotential or temperature out of every
 * accumulation at no extra pass), X_k = sum_j a[j] exp(-2 pi i jk / W), and
 *   P_0 = (pivot + Re X_0 / W)^2,   P_k = c_k (Re X_k^2 + Im X_k^2) / W^2 for 1 <= k <= K,   c_k = 2 except c_{W/2} = 1,
 * so that with K = W/2 sum_k P_k is the row's mean square (Parseval).  out [N][B][planes][K + 1] = sum_h band_weight[b][h] * P_k;
 * a row of weight exactly 0 adds nothing to its band.  Non-finite values are NOT detected: a NaN in a row makes every
 * wavenumber of that (item, plane) NaN in the bands whose weight for the row is non-zero (an infinity: NaN or infinite), and
 * nothing else.
 * basis_cos / basis_sin [W/2 + 1][K + 1]: cos / sin(2 pi ((j k) mod W) / W), float64 rounded once (the caller builds and keeps
 * them; score.spectrum_basis).  The transform is a folded real DFT (e[j] = a[j] + a[W - j], o[j] = a[j] - a[W - j]: half the
 * reduction length) on the f32-input MFMA with fp32 accumulation.  workspace >= pangu_zonal_spectrum_ws_bytes(N, planes, H, B, K)
 * = N * planes * ceil(H / 128) * B * (K + 1) * 4 bytes (host-only; PANGU_E_SHAPE for sizes out of range), 4-B aligned: per-row-tile
 * partials and one fixed-order reduce launch (tiles added in double), no atomics: every output is bit-identical from run to run,
 * and a column's value does not depend on K, N or the stride.  Two launches on `stream`, no host sync; everything is checked
 * before the first.
 * PANGU_E_NULL: a required pointer (all but minus); PANGU_E_SHAPE: N < 1, B outside 1..4, K outside 1..W/2, W % 4 != 0, W < 8,
 * W >= 2^15, a non-positive size, H*W >= 2^31, an item stride that is short or no multiple of 4, (N - 1) * stride + planes*H*W
 * > 2^40; PANGU_E_ARG: a workspace that is too small, or fields / minus / out / the basis tables not 16-B aligned. */
long long pangu_zonal_spectrum_ws_bytes(int N, int planes, int H, int B, int K);
int pangu_zonal_spectrum_f32(pangu_stream_t stream, const float* fields, long long item_stride, int N, const float* minus,
                             const float* band_weight, int B, const float* basis_cos, const float* basis_sin, int K,
                             float* out, void* workspace, long long workspace_bytes, int planes, int H, int W);

/* ---- bf16 variants (BASELINE configs[2], [4]) --------------------------------------------------------------
 * Activations and weight shadows are bf16 (raw uint16 bit patterns); biases, LayerNorm parameters, softmax and all
 * accumulation stay fp32.  Same semantics and layouts as the fp32 entry points above. */

/* C = act(A @ W^T + bias): A [M][K] bf16 (row stride lda), W [N][K] bf16, bias fp32 (may be NULL), C bf16 or fp32
 * (out_dtype = PANGU_BF16 / PANGU_F32), aux bf16 [M][N].  K % 8 == 0, N % 8 == 0. */
int pangu_linear_fwd_bf16(pangu_stream_t stream, const void* A, int lda, const void* W, const float* bias, void* C,
                          int ldc, int M, int N, int K, int act, void* aux, int out_dtype);

/* qkv, qkv_bias, esb, out bf16; lse fp32 (may be NULL). */
int pangu_window_attn_fwd_bf16(pangu_stream_t stream, const void* qkv, const void* qkv_bias, const void* esb, void* out,
                               float* lse, int Z, int H, int W, int C, int heads, int shifted);

/* The same attention with the QKV projection fused in (reference layers.py:365-374 + :378-415): q, k, v are computed
 * per (window, head) from the window's input rows x [tokens][C] (row stride ldx, bf16) and linear1 (w_qkv [3C][C] bf16,
 * b_qkv [3C] fp32) inside the kernel; the (tokens x 3C) qkv tensor is never materialised.  C = 192 or 384. */
int pangu_window_attn_qkv_fwd_bf16(pangu_stream_t stream, const void* x, int ldx, const void* w_qkv, const float* b_qkv,
                                   const void* esb, void* out, float* lse, int Z, int H, int W, int C, int heads,
                                   int shifted);

int pangu_ln_residual_fwd_bf16(pangu_stream_t stream, const void* y, const void* shortcut, int lds, const float* gamma,
                               const float* beta, void* out, int ldo, int N, int C, float branch_scale);
/* Projection + post-norm residual in one launch (inference path of layers.py:250-251):
 *   out[M,N] = shortcut[M,N] + LayerNorm(A[M,K] @ W[N,K]^T + bias) * gamma + beta,   N = 192 or 384 (the tile spans the row).
 * A, W, shortcut (dense, ld = N), out (row stride ldo) bf16; bias (may be NULL), gamma, beta fp32; statistics in fp32 on the
 * accumulators.  K % 8 == 0.  Replaces pangu_linear_fwd_bf16 + pangu_ln_residual_fwd_bf16 (branch scale 1). */
int pangu_linear_ln_residual_fwd_bf16(pangu_stream_t stream, const void* A, int lda, const void* W, const float* bias,
                                      const void* shortcut, const float* gamma, const float* beta, void* out, int ldo, int M,
                                      int N, int K);
/* Whole MLP branch + post-norm residual in one launch (inference path of reference models/layers.py:251 with
 * Mlp.forward :264-270 inside):
 *   out[M,C] = x[M,C] + branch_scale * ( LayerNorm( GELU(x W1^T + b1) W2^T + b2 ) * gamma + beta ),   C = 192 or 384.
 * x (row stride ldx), out (row stride ldo) bf16; b1 [4C], b2/gamma/beta [C] fp32; w_packed = the bf16 chunk image of
 * (W1 [4C][C], W2 [C][4C]) laid out as csrc/mlp_fused_bf16.hip documents (4C/32 chunks of 64*C elements).  The hidden
 * activation (M x 4C) never reaches memory.  Replaces two pangu_linear_fwd_bf16 + pangu_ln_residual_fwd_bf16. */
int pangu_mlp_ln_residual_fwd_bf16(pangu_stream_t stream, const void* x, int ldx, const void* w_packed, const float* b1,
                                   const float* b2, const float* gamma, const float* beta, void* out, int ldo, int M,
                                   int C, float branch_scale);
/* Training forward of the same branch (the bf16 counterpart of reference models/pangu_sample.py:45-77's forward through
 * layers.py:251, :264-270): as above, and the two tensors the backward needs leave from the registers they live in --
 *   pre [M][4C] bf16 (row stride ldp): x W1^T + b1 BEFORE the GELU;
 *   m   [M][C]  bf16 (row stride ldm): GELU(pre) W2^T + b2 BEFORE the LayerNorm.
 * The hidden activation h = GELU(pre) is not stored: pangu_linear_gelu_bwd_bf16 re-creates it in the backward. */
int pangu_mlp_ln_residual_train_fwd_bf16(pangu_stream_t stream, const void* x, int ldx, const void* w_packed,
                                         const float* b1, const float* b2, const float* gamma, const float* beta, void* out,
                                         int ldo, void* pre, int ldp, void* m, int ldm, int M, int C, float branch_scale);
/* Backward through Mlp.linear2 + GELU in one launch (reference layers.py:264-270 under autograd):
 *   dpre[M,N] = (A[M,K] @ W[N,K]^T) * gelu'(pre[M,N]),   h[M,N] = GELU(pre[M,N])
 * A = dm (row stride lda), W = linear2.weight^T laid out (N = 4C, K = C), pre dense [M][N]; dpre (row stride ldc) and h
 * (dense, may be NULL) bf16.  h feeds the weight gradient of linear2 (dW2 = dm^T h) and is transient. */
int pangu_linear_gelu_bwd_bf16(pangu_stream_t stream, const void* A, int lda, const void* W, void* dpre, int ldc, int M,
                               int N, int K, const void* pre, void* h);
int pangu_downsample_ln_fwd_bf16(pangu_stream_t stream, const void* x, int ldx, const float* gamma, const float* beta,
                                 void* out, int Z, int H, int W, int C);
int pangu_upsample_ln_fwd_bf16(pangu_stream_t stream, const void* y, const float* gamma, const float* beta, void* out,
                               int Z, int H2, int W2, int H, int Co);

/* fp32 fields -> bf16 GEMM operands; a_surface is [H4*W4][128] (columns 112..127 zero: K padded to a multiple of 64). */
int pangu_patch_embed_gather_bf16(pangu_stream_t stream, const float* input, const float* input_surface,
                                  const float* surface_mean, const float* surface_std, const float* upper_mean,
                                  const float* upper_std, const float* maps, const float* const_h, void* a_surface,
                                  void* a_upper, int LAT, int LON, int levels_reversed);

/* bf16 backward (configs[2]): operands / saved activations / activation gradients bf16; parameter gradients,
 * statistics and all accumulation fp32 (they feed the fp32 master weights).  Semantics as the fp32 entry points. */
int pangu_linear_wgrad_bf16(pangu_stream_t stream, const void* dC, int lddc, const void* A, int lda, float* dW,
                            float* db, int M, int N, int K);
/* The same product with a caller-owned scratch buffer (16-B aligned device memory, contents irrelevant before and after):
 * when it holds one fp32 partial tile per resident workgroup (N rounded up to whole tiles x K per token slab: <= 80 MB at the
 * model's shapes) the partial tiles are written there with plain stores (in MFMA register order) and summed into dW by a second
 * launch instead of 75 MB of fp32 atomics; too small or NULL = the entry above. */
int pangu_linear_wgrad_bf16_ws(pangu_stream_t stream, const void* dC, int lddc, const void* A, int lda, float* dW,
                               float* db, int M, int N, int K, float* workspace, long long workspace_bytes);
int pangu_window_attn_bwd_bf16(pangu_stream_t stream, const void* qkv, const void* qkv_bias, const void* esb,
                               const void* out, const float* lse, const void* dout, void* dqkv, float* dqkv_bias,
                               float* d_esb, int Z, int H, int W, int C, int heads, int shifted);
int pangu_ln_residual_bwd_bf16(pangu_stream_t stream, const void* dout, int lddo, const void* y, const float* gamma,
                               void* dy, float* dgamma, float* dbeta, int N, int C, float branch_scale);
int pangu_downsample_ln_bwd_bf16(pangu_stream_t stream, const void* dout, const void* x, int ldx, const float* gamma,
                                 void* dx, float* dgamma, float* dbeta, int Z, int H, int W, int C, const void* dx_add);
int pangu_upsample_ln_bwd_bf16(pangu_stream_t stream, const void* dout, const void* y, const float* gamma, void* dy,
                               float* dgamma, float* dbeta, int Z, int H2, int W2, int H, int Co);
int pangu_patch_recover_gather_bwd_bf16(pangu_stream_t stream, const float* d_output, const float* d_output_surface,
                                        void* dy_upper, void* dy_surface, int LAT, int LON);

/* bf16 weight shadows: every bf16 derived copy of the fp32 master weights re-made by ONE launch (the bf16 paths of
 * PanguModel compute on bf16 images of the reference's fp32 parameters -- pangu_model.py:9-48 -- which go stale at every
 * optimizer step, finetune_fully.py:121 / pangu_sample.py:75).  `jobs`: device memory, (n_jobs + 1) rows of 8 int64:
 *   [0] src0 (float*)  [1] src1 (float*, gather)  [2] dst (bf16*)  [3] idx (int32*, gather)  [4] n0  [5] n1  [6] mode
 *   [7] first block of the job; row n_jobs is a sentinel whose [7] = total_blocks.
 *   mode 0: dst[i] = bf16(src0[i]), i < n0 (4096 elements per block; src0 / dst 16-B aligned)
 *   mode 1: dst[c][r] = bf16(src0[r][c]), r < n0, c < n1 (one 64 x 64 tile per block)
 *   mode 2: e = idx[i]; dst[i] = bf16(e < n0 ? src0[e] : src1[e - n0]), i < n1 (4096 elements per block)
 * Rounding: to nearest even, as torch's float32 -> bfloat16 cast. */
int pangu_shadow_refresh_bf16(pangu_stream_t stream, const void* jobs, int n_jobs, long long total_blocks);

/* Training loss of the reference (models/pangu_sample.py:61-67, weights era5_data/config.py:45-46) in one pass per direction:
 *   loss = mean(|out - target| * w_upper[var]) + 0.25 * mean(|out_surface - target_surface| * w_surface[var])
 * out / target: [B][Vu][plane_u] fp32 (plane_u = levels * H * W), out_surface / target_surface: [B][Vs][plane_s]; w_upper [Vu],
 * w_surface [Vs] device fp32.  fwd: `partial` = scratch of pangu_weighted_l1_loss_blocks(..) floats; loss[0] = the loss,
 * loss[1] / loss[2] = the two means.  bwd: grad = device scalar (d loss); d_out = sign(out - target) * ((grad / n) * w[var])
 * in the order torch's autograd multiplies (surface: grad * 0.25 first), sign(0) = 0.
 * levels: the upper-air level count (plane_u % levels == 0): blocks never straddle a (sample, variable, level) plane.
 * The target side of the loop body is folded in (no separate pass over the 286 MB target):
 *   target_levels_reversed != 0: `target` is stored with its level axis in the file's (ascending) order (the reader's
 *     `[::-1]`, era5_data/utils_data.py:117, becomes an address: logical level l = plane levels-1-l);
 *   t_mean_upper / t_std_upper [Vu][levels] (logical level order), t_mean_surface / t_std_surface [Vs], all four or none:
 *     the targets arrive in physical units and are normalised on the fly, (t - mean) / std -- `normData`,
 *     era5_data/utils_data.py:315-321, called at models/pangu_sample.py:57.  NULL: the targets are already normalised. */
long long pangu_weighted_l1_loss_blocks(int B, int Vu, long long plane_u, int Vs, long long plane_s, int levels);
int pangu_weighted_l1_loss_fwd(pangu_stream_t stream, const float* out, const float* target, const float* out_surface,
                               const float* target_surface, const float* w_upper, const float* w_surface, float* partial,
                               float* loss, int B, int Vu, long long plane_u, int Vs, long long plane_s, int levels,
                               int target_levels_reversed, const float* t_mean_upper, const float* t_std_upper,
                               const float* t_mean_surface, const float* t_std_surface);
int pangu_weighted_l1_loss_bwd(pangu_stream_t stream, const float* out, const float* target, const float* out_surface,
                               const float* target_surface, const float* w_upper, const float* w_surface, const float* grad,
                               float* d_out, float* d_out_surface, int B, int Vu, long long plane_u, int Vs, long long plane_s,
                               int levels, int target_levels_reversed, const float* t_mean_upper, const float* t_std_upper,
                               const float* t_mean_surface, const float* t_std_surface);

/* Multi-step (rollout) fine-tuning: the gradient that enters the model's output at step k of a K-step chain, in ONE pass:
 *   d_out = [what pangu_weighted_l1_loss_bwd writes] + d_next * std[var][level]
 * d_next / d_next_surface (both or neither): d loss / d (physical input fields of step k+1), [B][Vu][plane_u] / [B][Vs][plane_s] in the
 * MODEL's level order (never reversed); the multiply by std is the adjoint of `normBackData` (out * std + mean,
 * era5_data/utils_data.py:324-330), which the forward's last kernel folds in (pangu_patch_recover_scatter_denorm).  The product
 * is rounded to fp32 before the add (what the two torch ops give).  std_upper [Vu][levels] (logical level order), std_surface [Vs]:
 * required when d_next is given.  d_out / d_out_surface MAY be the very buffers d_next / d_next_surface (elementwise, same index).
 * grad: device scalar, lead-time weight x upstream gradient.  d_next == NULL (the last step): bit-identical to
 * pangu_weighted_l1_loss_bwd.  Every other argument as there. */
int pangu_rollout_l1_seed_bwd(pangu_stream_t stream, const float* out, const float* target, const float* out_surface,
                              const float* target_surface, const float* w_upper, const float* w_surface, const float* grad,
                              const float* d_next, const float* d_next_surface, const float* std_upper, const float* std_surface,
                              float* d_out, float* d_out_surface, int B, int Vu, long long plane_u, int Vs, long long plane_s,
                              int levels, int target_levels_reversed, const float* t_mean_upper, const float* t_std_upper,
                              const float* t_mean_surface, const float* t_std_surface);

/* Fair-CRPS training loss over E ensemble members (2 <= E <= 16), one pass per direction (csrc/crps_loss.hip).  Per grid point,
 * x_e the members' normalised outputs, t the normalised target:
 *   c = (1/E) sum_e |x_e - t| - 1/(2E(E-1)) sum_e sum_f |x_e - x_f|
 *   loss = mean(w_upper[var] * a[h] * c) + 0.25 * mean(w_surface[var] * a[h] * c_surface)
 * members / members_surface: HOST arrays of E device pointers, member e's fields [B][Vu][levels][H][W] / [B][Vs][H][W] fp32 (the
 * outputs of E forwards; the entry copies the addresses into the kernel arguments).  target / target_surface, w_upper / w_surface,
 * target_levels_reversed and the four statistics: as for pangu_weighted_l1_loss_fwd.  lat_weight: H device floats, the weight a[h]
 * of latitude row h, or NULL for a = 1.  fwd: `partial` = scratch of pangu_fair_crps_loss_blocks(..) floats; loss[0] = the loss,
 * loss[1] / loss[2] = the two means; fp32 block partials summed by one fixed-order fp64 launch (no atomics: the same bits every
 * run).  bwd: grad = device scalar (d loss), k = 1/n_upper or 0.25/n_surface, sign(0) = 0:
 *   d_members[e] = grad * k * w[var] * a[h] * (sign(x_e - t)/E - sum_f sign(x_e - x_f) / (E(E-1)))
 * d_members / d_members_surface: HOST arrays of E device pointers; d_members[e] MAY be members[e] itself (every thread reads all E
 * values of an element before its first store).  A 16-byte vector path runs when W % 4 == 0 and every field is 16-byte aligned,
 * a scalar path otherwise.  PANGU_E_NULL: a NULL pointer (array entries included; statistics not all four or none), PANGU_E_ARG:
 * E outside 2..16, PANGU_E_SHAPE: a non-positive size, H * W or the block count out of range. */
long long pangu_fair_crps_loss_blocks(int E, int B, int Vu, int levels, int Vs, int H, int W);
int pangu_fair_crps_loss_fwd(pangu_stream_t stream, const float* const* members, const float* const* members_surface, int E,
                             const float* target, const float* target_surface, const float* w_upper, const float* w_surface,
                             const float* lat_weight, float* partial, float* loss, int B, int Vu, int levels, int Vs, int H, int W,
                             int target_levels_reversed, const float* t_mean_upper, const float* t_std_upper,
                             const float* t_mean_surface, const float* t_std_surface);
int pangu_fair_crps_loss_bwd(pangu_stream_t stream, const float* const* members, const float* const* members_surface, int E,
                             const float* target, const float* target_surface, const float* w_upper, const float* w_surface,
                             const float* lat_weight, const float* grad, float* const* d_members, float* const* d_members_surface,
                             int B, int Vu, int levels, int Vs, int H, int W, int target_levels_reversed,
                             const float* t_mean_upper, const float* t_std_upper, const float* t_mean_surface,
                             const float* t_std_surface);

/* Host side of the input pipeline (the idea of reference era5_data/utils_data.py:16-51 and the four
 * `.to(device)` of models/pangu_sample.py:41-43): copy `bytes` from the loader's pageable memory into a page-locked staging
 * buffer with up to `threads` host threads (each one contiguous 4 KB-aligned span; < 4 MB per thread is not split).  Pure
 * host code, no stream, returns when the copy is complete. */
int pangu_host_copy(void* dst, const void* src, long long bytes, int threads);

/* Output side of the forecast loop (data.HostDrain): a field of `planes` planes of `plane_elems` contiguous fp32 values each is
 * packed on the device to int16 with one (scale, offset) per plane -- ERA5 NetCDF's `scale_factor` / `add_offset` storage -- or
 * staged as fp32, before the copy engine takes it to page-locked host memory.
 *   value:      v = src * mul[s] + add[s] in two roundings (multiply, then add: `normBackData`, reference
 *               era5_data/utils_data.py:324-330) with mul / add fp32 [planes] indexed by SOURCE plane s, both or neither (NULL: v = src);
 *   addressing: levels = 0: output plane p reads source plane p; levels = L (planes % L == 0): output plane v*L + l reads source
 *               plane v*L + (L-1-l) -- the reader's level reversal (utils_data.py:117);
 *   packing:    over the FINITE v of a plane: offset = (max + min) / 2, scale = (max - min) / 65534, scale = 1 when that is 0 (a
 *               constant plane, an underflowing range) or when the plane has no finite value (then offset = 0);
 *               q = clamp(rint((v - offset) * (1 / scale)), -32767, 32767); a non-finite v packs to the fill value -32768.
 *               For finite v, in exact arithmetic on the stored fp32 scale / offset:
 *                 |q * scale + offset - v| <= 0.5 * scale * (1 + 2^-10) + 4 * 2^-24 * max(|min|, |max|),
 *               min packs to -32767 and max to +32767.  A plane whose range overflows fp32 is outside the contract.
 *   outputs:    packed int16 [planes][plane_elems], scale_offset fp32 [planes][2] = (scale, offset), nonfinite int32 [planes] = the
 *               number of non-finite v; all indexed by OUTPUT plane.
 * pangu_pack_planes_i16 is two launches on `stream` (per-workgroup min / max / count partials into `workspace`, then quantise; no
 * atomics, nothing has to be zeroed, bit-identical from run to run); workspace >= pangu_pack_i16_ws_bytes(planes, plane_elems)
 * bytes (PANGU_E_ARG otherwise), 4-B aligned.  pangu_pack_i16_ws_bytes is host-only and returns PANGU_E_SHAPE for sizes out of range
 * (planes <= 0, plane_elems <= 0 or >= 2^31, more than 2^31 - 1 workgroups).  pangu_stage_planes_f32: dst[p] = v, fp32, one launch.
 * 16-B loads and stores run where a plane's base allows it; any plane_elems and any 4-B (src, dst) / 2-B (packed) aligned base work.
 * pangu_unpack_i16_host is pure host code (no stream): dst = (float)q * scale + offset in fp32 (two roundings), the fill value ->
 * NaN, split over up to `threads` host threads (contiguous spans; < 1 M values per thread is not split). */
long long pangu_pack_i16_ws_bytes(int planes, long long plane_elems);
int pangu_pack_planes_i16(pangu_stream_t stream, const float* src, const float* mul, const float* add, short* packed,
                          float* scale_offset, int* nonfinite, void* workspace, long long workspace_bytes, int planes,
                          long long plane_elems, int levels);
int pangu_stage_planes_f32(pangu_stream_t stream, const float* src, const float* mul, const float* add, float* dst, int planes,
                           long long plane_elems, int levels);
int pangu_unpack_i16_host(float* dst, const short* src, const float* scale_offset, int planes, long long plane_elems, int threads);

/* First-order conservative remapping of `planes` planes [H_in][W_in] to a coarser grid [H_out][W_out] of the same family (latitudes
 * 90 - j * 180 / (H - 1), poles included; longitudes i * 360 / W), one launch on `stream`, no workspace, no atomics, bit-identical
 * from run to run:
 *   dst[p][J][I] = sum_s lon_w[I][s] * ( sum_t lat_w[J][t] * v[q][lat_start[J] + t][(lon_start[I] + s) mod W_in] ),
 * with v = src * mul[q] + add[q] in two roundings, mul / add fp32 [planes] indexed by SOURCE plane q, both or neither (NULL: v =
 * src), and q = p (levels = 0) or the level-reversed plane (levels = L), exactly as for pangu_stage_planes_f32.  Each sum is taken
 * in fp32 in tap order: the first product, then one fma per further tap, latitude first; a row of one tap of weight 1 returns its
 * input bit for bit.  Non-finite values are not masked: they propagate to every output cell whose stencil holds one.
 *   lat_start / lat_count int32 [H_out], lat_w fp32 [H_out][lat_taps] (zero-padded); lon_start / lon_count int32 [W_out], lon_w
 *   fp32 [W_out][lon_taps]; device memory, built by score.regrid_plan.
 * The tables are TRUSTED (the caller's contract, not checked): 1 <= lat_count[J] <= lat_taps, 0 <= lat_start[J] and lat_start[J] +
 * lat_count[J] <= H_in; 1 <= lon_count[I] <= lon_taps, -W_in < lon_start[I] < W_in (read modulo W_in).
 * Planes whose rows are 16-B aligned (W_in % 4 == 0 and a 16-B aligned plane base) are read with 16-B loads, others with 4-B loads.
 * Checked before the launch -- PANGU_E_NULL: a NULL pointer (mul and add: one without the other); PANGU_E_SHAPE: a non-positive
 * size, H_out > H_in, W_out > W_in, lat_taps or lon_taps outside 1..16, levels < 0 or planes % levels != 0, W_in > 16384 (one row
 * is staged in LDS), H_in * W_in >= 2^31, planes * H_out >= 2^31; PANGU_E_ARG: src or dst not 4-B aligned. */
int pangu_regrid_planes_f32(pangu_stream_t stream, const float* src, const float* mul, const float* add, float* dst, int planes,
                            int H_in, int W_in, int H_out, int W_out, const int* lat_start, const int* lat_count,
                            const float* lat_w, int lat_taps, const int* lon_start, const int* lon_count, const float* lon_w,
                            int lon_taps, int levels);

/* Regional scorecard sums of a deterministic forecast: every latitude-weighted sum behind bias, MAE, RMSE, ACC (uncentred and
 * centred), forecast activity and wind-vector RMSE, for 1 <= R <= 8 regions, in one streaming pass over pred and target
 * [planes][H][W] fp32 in physical units (csrc/scorecard.hip pins the definitions).  W % 4 == 0.
 *   target_levels = L > 1: target plane v*L + l is read at v*L + (L-1-l), the level reversal of pangu_regrid_planes_f32 (planes % L
 *                   == 0); 0 or 1: no reversal;
 *   clim_kind     0: no climatology, c = 0 (clim is not read); 1: one scalar per plane, clim [planes]; 2: a field, clim
 *                   [planes][H][W], indexed like pred;
 *   region_bits   [H][W] bytes shared by all planes: bit r of a point's byte says that the point belongs to region r < R (higher
 *                   bits are ignored); NULL: one region that holds every point (R must be 1);
 *   sums          [planes][R][10] doubles.  With d = p - t, a = p - c, b = t - c (one fp32 rounding each) and w = lat_weight[h], over
 *                   the points of the region:
 *                     [0] sum w     [1] sum w d    [2] sum w |d|    [3] sum w d^2    [4] sum w a
 *                     [5] sum w b   [6] sum w a b  [7] sum w a^2    [8] sum w b^2    [9] the number of points.
 * Membership is a select, never a product with 0: a non-finite value at a point reaches the sums of exactly the regions that hold
 * the point; an empty region gives ten zeros.  Each (plane, slab of 32 rows) writes its fp32 partials (the count as an integer) to
 * workspace, >= pangu_scorecard_ws_bytes(planes, H, R) = planes * ceil(H / 32) * R * 40 bytes (host-only; PANGU_E_SHAPE for sizes out
 * of range); one reduce launch adds the slabs in slab order in double.  No atomics: every output is bit-identical from run to run,
 * and a plane's sums do not depend on which other planes are in the launch.  Two launches on `stream`, no host sync; everything is
 * checked before the first.
 * PANGU_E_NULL: a required pointer (pred, target, lat_weight, sums, workspace), clim with clim_kind != 0, region_bits == NULL with
 * R != 1; PANGU_E_SHAPE: W % 4, a non-positive size, H*W >= 2^31, R outside 1..8, target_levels < 0 or planes % target_levels != 0,
 * planes * ceil(H / 32) >= 2^31; PANGU_E_ARG: clim_kind outside 0..2, a workspace that is too small, or a pointer that misses its
 * alignment: 16 B for pred, target, a clim field and the workspace, 8 B for sums, 4 B for region_bits, lat_weight and clim scalars. */
long long pangu_scorecard_ws_bytes(int planes, int H, int R);
int pangu_scorecard_sums_f32(pangu_stream_t stream, const float* pred, const float* target, int target_levels, const float* clim,
                             int clim_kind, const float* lat_weight, const unsigned char* region_bits, int R, double* sums,
                             void* workspace, long long workspace_bytes, int planes, int H, int W);

/* Event verification of a deterministic forecast: the contingency table of the events pred > thr / target > thr and the sums of the
 * Fractions Skill Score over square neighbourhoods, in one streaming pass over pred and target [planes][H][W] fp32 in physical units
 * (csrc/events.hip pins the definitions).
 *   Events      f = pred > thresholds[t][p], o = target > thresholds[t][p], strict; thresholds [T][planes], 1 <= T <= 4.  +inf is an
 *               event that never happens; a comparison with NaN is false (non-finite values are not detected).
 *   target_levels  as for pangu_scorecard_sums_f32: L > 1 reads target plane v*L + l at v*L + (L-1-l) (planes % L == 0).
 *   Domain      a point is in the domain iff domain_bits ([H][W] bytes, e.g. a scorecard region mask) is NULL or bit domain_bit
 *               (0..7) of its byte is set.  The domain selects CENTRE points only: every grid point feeds neighbourhood counts.
 *   counts      [T][planes][4] over domain points: hits (f and o), false alarms (f, not o), misses (o, not f), correct negatives:
 *               exact integers.  wsums [T][planes][4]: the same with every point weighted by lat_weight[h], in double.
 *   radii       HOST memory, 1 <= N <= 4 strictly increasing values, 0 <= r <= 32 and 2r+1 <= W.  Radius r is the (2r+1) x (2r+1) box
 *               of grid points around (h, w): columns wrap modulo W, rows outside 0..H-1 are absent, rows_h = min(h+r, H-1) -
 *               max(h-r, 0) + 1, n_h = rows_h (2r+1); cf(h,w), co(h,w) are the integer numbers of f and o events in the box.
 *   fss         [T][planes][N][2] = { sum_h s_h A_h, sum_h s_h B_h }, s_h = (double)lat_weight[h] / ((double)n_h n_h), A_h = sum over
 *               domain points w of (cf - co)^2, B_h = sum over domain points w of (cf^2 + co^2), exact 64-bit integer row sums.
 *               FSS = 1 - fss[0] / fss[1]; at r = 0, fss[0] = false alarms + misses and fss[1] = 2 hits + false alarms + misses,
 *               weighted.
 * Each (plane, row) writes its integers to workspace, >= pangu_event_scores_ws_bytes(planes, H, T, N) = planes * H * (1 + 3T + 2TN)
 * * 8 bytes (host-only; PANGU_E_SHAPE for sizes out of range); a second launch applies the weights in double in a fixed order.  No
 * atomics: every output is bit-identical from run to run and does not depend on which other planes, thresholds or radii are in
 * the call.  Two launches on `stream`, no host sync; everything is checked before the first.
 * PANGU_E_NULL: pred, target, thresholds, radii, lat_weight, counts, wsums, fss or workspace; PANGU_E_SHAPE: a non-positive size,
 * W % 4, W > 4096, H*W >= 2^31, T or N outside 1..4, a radius outside 0..32, not above its predecessor or with 2r+1 > W,
 * target_levels < 0 or planes % target_levels != 0, planes * ceil(H / 32) >= 2^31; PANGU_E_ARG: domain_bit outside 0..7, a workspace
 * that is too small, or a pointer that misses its alignment: 16 B for pred, target and the workspace, 8 B for counts, wsums and fss,
 * 4 B for thresholds, lat_weight and domain_bits. */
long long pangu_event_scores_ws_bytes(int planes, int H, int T, int N);
int pangu_event_scores_f32(pangu_stream_t stream, const float* pred, const float* target, int target_levels,
                           const float* thresholds, int T, const int* radii, int N, const float* lat_weight,
                           const unsigned char* domain_bits, int domain_bit, unsigned long long* counts, double* wsums, double* fss,
                           void* workspace, long long workspace_bytes, int planes, int H, int W);

/* Lead-window statistics: fold ONE lead's field src [planes][plane_elems] fp32 into the accumulators of ONE window of leads, one
 * launch on `stream`, no workspace, no atomics (csrc/leadstats.hip pins the definitions).  v = src * mul[q] + add[q] in two
 * roundings, mul / add fp32 [planes] indexed by SOURCE plane q, both or neither (NULL: v = src), and q = p (levels = 0) or the
 * level-reversed plane (levels = L), exactly as for pangu_regrid_planes_f32.  Every output is [planes][plane_elems], indexed by
 * output plane p, and may be NULL (not kept); per element, with `lead` in 0..254:
 *   first != 0 (the window's first lead): outputs are assigned and never read, so nothing needs zeroing:
 *       sum = v; vmin = vmax = v; when_min = when_max = lead; per threshold t: e = (v > thr[t][p]), count = run = longest = e;
 *   first == 0:
 *       sum = sum + v (one fp32 add: the left-to-right fp32 sum in lead order);
 *       if (v < vmin || v != v) { vmin = v; when_min = lead; }, the same with > for vmax / when_max: a NaN takes the extreme and no
 *       number takes it back, a tie (signed zeros included) keeps the earlier lead, +-inf are numbers;
 *       e = (v > thr[t][p]) (false for NaN); count += e; run = e ? run + 1 : 0; longest = max(longest, run).
 *   thr fp32 [T][planes], 0 <= T <= 4, +inf: no event; count, run, longest bytes [T][planes][plane_elems]; when_min, when_max bytes.
 *   A window holds at most 255 leads, so no byte counter wraps.
 * Planes whose arrays all have one phase (the same number of elements, 0..3, up to a 16-B boundary of the fp32 fields and a 4-B
 * boundary of the byte fields) are accessed 16 B / 4 B per lane after a scalar head; other planes 4 B / 1 B per lane.  Outputs are
 * bit-identical from run to run and independent of the other planes of the launch.
 * Checked before the launch -- PANGU_E_NULL: src; mul without add or the reverse; thr with T > 0.  PANGU_E_SHAPE: a non-positive
 * size, plane_elems >= 2^31, levels < 0 or planes % levels != 0, T outside 0..4, lead outside 0..254, planes * ceil(plane_elems /
 * 2048) >= 2^31.  PANGU_E_ARG: no output requested; when_min without vmin or when_max without vmax; longest without run; T > 0 with
 * neither count nor longest; T == 0 with count, run or longest; an fp32 pointer that is not 4-B aligned. */
int pangu_lead_stats_update_f32(pangu_stream_t stream, const float* src, const float* mul, const float* add, float* sum, float* vmin,
                                float* vmax, unsigned char* when_min, unsigned char* when_max, const float* thr, int T,
                                unsigned char* count, unsigned char* run, unsigned char* longest, int planes, long long plane_elems,
                                int levels, int lead, int first);

/* The observation operator: bilinear interpolation of `planes` planes src [planes][H][W] fp32 to N points, and the departure
 * statistics of the interpolated forecast against observations at those points (csrc/points.hip pins the definitions).  Any W: the
 * gather uses 4-B loads.  v = src * mul[q] + add[q] in two roundings, mul / add fp32 [planes] indexed by SOURCE plane q, both or
 * neither (NULL: v = src), and q = p (levels = 0) or the level-reversed plane (levels = L), exactly as for pangu_regrid_planes_f32;
 * out, obs and departures are [planes][N], indexed by output plane p.
 *   The plan (device memory, built by score.point_plan): row, col int32 [N], the grid node north-west of the point, and wy, wx fp32
 *   [N], the weights of the next row r1 = min(row + 1, H - 1) and of the next column c1 = (col + 1) mod W.  Every operation rounded
 *   once to fp32, no contraction:
 *     line(j) = wx == 0 ? v[j][col] : fl(fl(v[j][col] * fl(1 - wx)) + fl(v[j][c1] * wx))
 *     f       = wy == 0 ? line(row) : fl(fl(line(row) * fl(1 - wy)) + fl(line(r1) * wy))
 *   A tap of weight zero is a select, never a product: a non-finite value at a node reaches exactly the points whose stencil holds
 *   the node with a non-zero weight, and a point on a node returns the node's value bit for bit.
 * The plan arrays are TRUSTED (the caller's contract, not checked): 0 <= row < H, 0 <= col < W, 0 <= wy, wx < 1 and wy == 0 where row
 * == H - 1.  (An index outside the grid is clamped into it: a broken plan gives wrong values, not an access outside the plane.)
 * pangu_sample_points_f32 writes f to out, one launch on `stream`, no workspace.
 * pangu_point_scores_f32: c = clim[p] (clim fp32 [planes], indexed by output plane; NULL: c = 0), d = f - o, a = f - c, b = o - c, one
 * fp32 rounding each, and the products rounded to fp32.  A point is valid for a plane iff its observation is not NaN (the marker of a
 * missing report; infinities are values).
 *   departures   optional (NULL: not kept): d, NaN where the observation is missing;
 *   region_bits  [N] bytes shared by all planes: bit r of a point's byte says that the point belongs to region r < R (higher bits are
 *                ignored); NULL: one region that holds every point (R must be 1);
 *   sums         [planes][R][10] doubles, the layout of pangu_scorecard_sums_f32 with weight 1, over the valid points of the region:
 *                  [0] n    [1] sum d    [2] sum |d|    [3] sum d^2    [4] sum a    [5] sum b    [6] sum a b    [7] sum a^2
 *                  [8] sum b^2    [9] n;  [0] and [9] are exact integers.
 * Membership and validity are selects; a region with no valid point gives ten zeros.  Each (plane, chunk of 1024 points) writes its
 * fp32 partials (the counts as integers) to workspace, >= pangu_point_scores_ws_bytes(planes, N, R) = planes * ceil(N / 1024) * R * 40
 * bytes (host-only; PANGU_E_SHAPE for sizes out of range); a second launch adds the chunks in chunk order in double.  No atomics:
 * every output is bit-identical from run to run, and a plane's outputs do not depend on which other planes are in the launch.  Two
 * launches on `stream`, no host sync; everything is checked before the first.
 * PANGU_E_NULL: a required pointer (src, the four plan arrays, out; obs, sums, workspace), mul without add or the reverse, region_bits
 * == NULL with R != 1; PANGU_E_SHAPE: a non-positive size, H < 2, H*W >= 2^31, planes * N >= 2^31, R outside 1..8, levels < 0 or planes
 * % levels != 0; PANGU_E_ARG: a workspace that is too small, or a pointer that misses its alignment: 8 B for sums, 4 B for the other
 * fp32 / int32 arrays and the workspace. */
int pangu_sample_points_f32(pangu_stream_t stream, const float* src, const float* mul, const float* add, const int* row,
                            const int* col, const float* wy, const float* wx, float* out, int planes, int H, int W, int N,
                            int levels);
long long pangu_point_scores_ws_bytes(int planes, int N, int R);
int pangu_point_scores_f32(pangu_stream_t stream, const float* src, const float* mul, const float* add, const int* row,
                           const int* col, const float* wy, const float* wx, const float* obs, const float* clim,
                           const unsigned char* region_bits, int R, float* departures, double* sums, void* workspace,
                           long long workspace_bytes, int planes, int H, int W, int N, int levels);

/* Adam over a whole list of tensors in ONE launch (reference finetune_fully.py:121 torch.optim.Adam, stepped at
 * models/pangu_sample.py:75): p, grad, exp_avg, exp_avg_sq fp32, updated in place with the arithmetic of torch's fused Adam
 * (L2 weight decay added to the gradient, bias corrections, eps outside the root; doubles where that code uses doubles) -- bit
 * identical to torch.optim.Adam(fused=True).  `jobs`: device memory, (n_jobs + 1) rows of 8 int64:
 *   [0] param  [1] grad (0 = an all-zero gradient that is never read)  [2] exp_avg  [3] exp_avg_sq  [4] bf16 image of the updated param to write as well, or 0  [5] n
 *   [6] 0 = the call's bias corrections, else float bits of (1 - beta1^step) | float bits of sqrt(1 - beta2^step) << 32 (tensors
 *   at different step counts)   [7] first block (4096 elements per block); row n_jobs: sentinel, [7] = total_blocks. */
int pangu_adam_step_multi(pangu_stream_t stream, const void* jobs, int n_jobs, long long total_blocks, double lr, double beta1,
                          double beta2, double weight_decay, double eps, float bias_correction1, float bias_correction2_sqrt);

/* Global-norm gradient clipping, an accumulation scale and a non-finite-step guard for the Adam above, over the SAME job table and
 * without touching the gradients or waiting on the host.  Three launches replace the one:
 *   1. pangu_grad_sumsq_multi, once per table: partials[b] = sum of grad^2 over table block b, accumulated in double in a fixed
 *      order (no atomics: bit-identical from run to run); a row with grad = 0 contributes 0.  `partials`: total_blocks doubles.
 *   2. pangu_grad_clip_state, once: adds `n_partials` doubles (the partials of every table, written next to each other) and writes
 *      the 24-byte device record `state`:
 *        +0  float  norm           = fl32(grad_scale * sqrt(sumsq)), the norm of the scaled gradient before clipping
 *        +4  float  multiplier     = fl32(grad_scale) * min(1.0f, fl32(max_norm) / (norm + 1e-6f)) with `clip` (the fp32 arithmetic
 *                                    of torch.nn.utils.clip_grad_norm_; a NaN stays a NaN), else fl32(grad_scale)
 *        +8  int    skip           = 1 when `skip_nonfinite` and sumsq is NaN or Inf, else 0
 *        +16 int64  skipped_total += skip (the record must be zeroed once by its owner)
 *   3. pangu_adam_step_multi_scaled, once per table: pangu_adam_step_multi on grad * multiplier (the product rounded to float, as
 *      if the gradient had been scaled in place).  With skip = 1 neither the parameters nor the moments are written; a row's bf16
 *      image [4] is still written, from the unchanged parameter.
 * max_norm must be > 0 when `clip`, grad_scale finite and > 0 (PANGU_E_ARG otherwise); counts as for pangu_adam_step_multi. */
int pangu_grad_sumsq_multi(pangu_stream_t stream, const void* jobs, int n_jobs, long long total_blocks, void* partials);
int pangu_grad_clip_state(pangu_stream_t stream, const void* partials, long long n_partials, void* state, int clip, double max_norm,
                          double grad_scale, int skip_nonfinite);
int pangu_adam_step_multi_scaled(pangu_stream_t stream, const void* jobs, int n_jobs, long long total_blocks, double lr, double beta1,
                                 double beta2, double weight_decay, double eps, float bias_correction1, float bias_correction2_sqrt,
                                 const void* state);

/* Rehearsal tool (not on the product path): copy `bytes` (multiple of 16, 16-B aligned pointers) device to device with a grid of
 * exactly `workgroups` 256-thread workgroups -- the HBM traffic / CU footprint of a collective on its own stream, for measuring how
 * much a bucketed gradient all-reduce (reference era5_data/utils_dist.py:125-134 semantics) slows the backward kernels it overlaps. */
int pangu_traffic_copy(pangu_stream_t stream, const void* src, void* dst, long long bytes, int workgroups);

#ifdef __cplusplus
}
#endif
#endif /* PANGU_HIP_H */
