/* bbbp_hip.h -- C ABI of libbbbp_hip.so, the MI355X (gfx950) implementation of the neural hot path of
 * FengDushuo/BBBP-Multi-Modal-Deep-Ensemble-Framework.
 *
 * The reference has no FFI of its own: its hot path is stock torch.nn modules called from Python
 * (SURVEY.md 8b).  These entry points are therefore what a binding for that path would call in
 * place of ATen; each one cites the reference statement(s) it replaces, relative to /root/reference/,
 * with R = Models/multi_input_data_regression_opt_transformer_cnn_20250113.py.
 *
 * Conventions: every pointer is a DEVICE pointer to fp32 data unless typed otherwise; tensors are
 * row-major contiguous in the reference's own layouts (NCHW images, [out,in] Linear weights);
 * `stream` is a hipStream_t (NULL = default stream); work is enqueued, never synchronised;
 * scratch memory is caller-provided (`workspace`, sized by the *_workspace_bytes functions);
 * every function returns 0 on success or a BBBP_ERR_* code, with text in bbbp_last_error();
 * nothing throws across the ABI.  No torch types appear anywhere.
 */
#ifndef BBBP_HIP_H
#define BBBP_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BBBP_OK 0
#define BBBP_ERR_ARG 1
#define BBBP_ERR_HIP 2
#define BBBP_ERR_WORKSPACE 3

#define BBBP_ACT_NONE 0
#define BBBP_ACT_RELU 1
#define BBBP_ACT_TANH 2

int bbbp_abi_version(void);
const char* bbbp_last_error(void);

/* ---- dense GEMM + bias + activation (+ residual) -------------------------------------------
 * C[M,N] = act(alpha * op(A) op(B) + bias[n]) + residual[M,N]; op by transA/transB:
 *   (0,1) A[M][K] B[N][K]: nn.Linear forward           R:79-82, 92, 98-107; nn.MultiheadAttention in/out proj R:75-78
 *   (0,0) A[M][K] B[K][N]: input gradients, P.V        autograd of the above (loss.backward(), R:190)
 *   (1,0) A[K][M] B[K][N]: weight gradients            idem
 * batch > 1 runs `batch` independent products with the given element strides (attention heads). */
size_t bbbp_gemm_workspace_bytes(int M, int N, int K, int batch);
int bbbp_gemm_f32(void* stream, int transA, int transB, int M, int N, int K, float alpha,
                  const float* A, int lda, const float* B, int ldb, float* C, int ldc,
                  const float* bias, const float* residual, int ldr, int act,
                  int batch, long strideA, long strideB, long strideC, long strideR,
                  void* workspace, size_t workspace_bytes);

/* One product of a grouped launch: the bbbp_gemm_f32 arguments as a struct, plus an optional gate: the result is
 * multiplied by gate_scale where gate[m][n] > 0 and by 0 elsewhere (after bias/act, before the residual) -- the
 * ReLU(+dropout) backward of linear1 (R:75-78 under loss.backward(), R:190) folded into the input-gradient GEMM. */
typedef struct bbbp_gemm_desc {
    int transA, transB, M, N, K;
    float alpha;
    const float* A; int lda;
    const float* B; int ldb;
    float* C; int ldc;
    const float* bias;
    const float* residual; int ldr;
    int act;
    const float* gate; int ldg; float gate_scale;
    int batch;
    long strideA, strideB, strideC, strideR, strideG;
    int gate_after_residual;      /* 0: gate(act(..)) + residual;  1: gate(act(..) + residual) */
    float* asum;                  /* optional, layout A^T B only (a Linear's weight gradient dW = dY^T X): asum[m] = sum_k A[k][m], the
                                     matching bias gradient, produced by the same MFMAs through a virtual all-ones column N of B.
                                     Honoured by the small-product path only: ask bbbp_gemm_folds_asum first. */
    float drop_p;                 /* optional dropout of the OUTPUT, applied after bias/act (before gate/residual): element (m, n) is
                                     scaled by the keep-scale of element m * N + n of Philox stream drop_seed -- the stream bbbp_dropout
                                     draws for a contiguous [M][N] tensor, so act + dropout of linear1 (R:75-78, train mode) is one launch.
                                     0 = off.  Small-product path only (bbbp_gemm_folds_asum(M, N, K, batch) == 1). */
    unsigned long long drop_seed;
} bbbp_gemm_desc;
/* 1 when a product of this shape (layout A^T B) takes the path that honours bbbp_gemm_desc.asum. */
int bbbp_gemm_folds_asum(int M, int N, int K, int batch);
/* `count` independent products (outputs must not alias another product's operands).  Products that become ready
 * together -- dV | dP and dQ | dK of the attention backward -- go out as ONE launch when both are small; anything
 * else runs back to back on `stream`.  Results are identical to `count` bbbp_gemm_f32 calls. */
int bbbp_gemm_f32_grouped(void* stream, const bbbp_gemm_desc* problems, int count, void* workspace, size_t workspace_bytes);
/* Which kernel family a product of this layout and shape runs on, under the process's BBBP_GEMM_* settings (host side, no GPU work):
 * 0 small-product path, 1 64 x 64 split-bf16 tile, 2 128 x 128 split-bf16 tile, 3 128 x 128 f32 tile, 4 its short-K variant, 5 64 x 64 f32 tile,
 * 6 weight-resident split-bf16 form (A B with K <= 128: one column block of B per work-group, every row tile of A streamed past it);
 * -1 for sizes or a layout bbbp_gemm_f32 rejects.  For A/B scripts and tests; a caller never needs it to run a product. */
int bbbp_gemm_kernel_form(int transA, int transB, int M, int N, int K, int batch);

/* ---- Conv2d(k3,s1,p1) + ReLU + MaxPool2d(2,2), NCHW ------------------------------------------
 * forward: R:85-87 (3->32, 128x128) and R:88-90 (32->64, 64x64).  y is the pooled output,
 * mask[B][cout][H/2][W/2] (u8) records the arg-max of each 2x2 window (0..3, PyTorch first-max order)
 * or 4 where the ReLU is inactive; backward consumes it instead of the pre-pool activation.  The forward's `mask` may be NULL
 * (round 4): a forward-only call (eval loop R:195-203, screening) keeps no decisions -- the engine's inference plans pass NULL.
 * bwd_data / bwd_weight: autograd of the same statements under loss.backward() (R:190). */
size_t bbbp_conv3x3_workspace_bytes(int B, int cin, int cout, int H, int W);
/* Measurement aid (bench.py): shader-clock cycles and 100 MHz wall ticks that work-group 0 of the most recent
 * forward / data-gradient conv launch ran for (synchronises the device). */
int bbbp_conv_last_clock(unsigned long long* shader_cycles, unsigned long long* ticks_100mhz);
/* Selects the algorithm of the 32->64 @ 64x64 stage (R:88-90).  bit 0 = forward, bit 1 = data gradient run as Winograd
 * F(2x2,3x3) in float32 (2.25x fewer multiplies, same tensors and mask, results within 1e-6 of the direct form).
 * bit 2 = forward, bit 3 = data gradient, bit 4 = weight gradient run as the direct implicit GEMM on the bf16 matrix pipe with
 * every float32 operand split into three bf16 pieces (six bf16 products per float32 product, float32 accumulate: float32
 * accuracy, csrc/conv_b3.hip); these bits take precedence over the Winograd bits.  bit 5 = the weight gradient of the 3->32 @
 * 128x128 stage (R:85-87) in the same split-bf16 form; bit 6 = that stage's forward (csrc/conv_b3c1.hip: channel-innermost LDS strip,
 * in-lane pooling windows).  Inside bbbp_mixed_forward the engine keeps the first stage's forward on the f32 kernel while a training
 * step's encoder chain runs beside it (the split-bf16 kernel leaves that chain no wave slots: measured slower for the step), so bit 6
 * acts on forward-only (inference-plan) passes -- eval loops, screening --, the encoder-less two-branch model and the op-level entry point.
 * 0 = direct implicit GEMM on the f32 MFMA everywhere.  Initial value: environment BBBP_CONV_WINOGRAD, else 252.
 * bit 7 (128, round 3): conv2's split-bf16 weight gradient on the 2:4 structured-sparse MFMA (v_smfmac_f32_32x32x32_bf16): the pooled
 * gradient expanded through the arg-max mask has at most one nonzero per pixel pair, so its compressed form is the pooled tensor itself
 * -- half the matrix-pipe time, same six piece products, same float32 accuracy; bit 8 (256): its 4-wave form wherever it runs (tests). */
int bbbp_set_conv_winograd(int mask);
int bbbp_get_conv_winograd(void);
/* Which kernel form a conv call of this stage runs on right now: under the current mask, the calling thread's two preferences
 * (bbbp_set_conv2_fwd_pipe, bbbp_set_conv_wgrad_beside_encoder) and the process's BBBP_C* settings (host side, no GPU work).
 * op: 0 forward, 1 data gradient, 2 weight gradient; hw: the input map's height = width.
 * 0 direct implicit GEMM on the f32 MFMA, 1 Winograd F(2x2,3x3), 2 split-bf16, 3 its software-pipelined kernel (64 x 64 maps),
 * 4 split-bf16 of the 3->32 stage (weight gradient, or the phase-by-phase forward), 5 that stage's software-pipelined forward,
 * 6 dense split-bf16 weight gradient, 7 / 8 the structured-sparse weight gradient with 8 / 4 waves;
 * -1 for a stage the entry points reject, the data gradient of a 3-channel stage included.
 * For A/B scripts and tests; a caller never needs it to run a conv. */
int bbbp_conv_kernel_form(int op, int cin, int cout, int hw);
/* Measurement aid: with BBBP_WINO_PROBE=1 in the environment the Winograd kernels stamp the shader clock at phase boundaries;
 * phases4 = cycles work-group 0 spent in {accumulator init, k-steps, stage hand-over, output transform} of the last launch. */
int bbbp_conv_winograd_phases(unsigned long long* phases4);
/* Same for the split-bf16 kernels (BBBP_B3_PROBE=1): [0] global-load issue, [1] MFMA block, [2] split + LDS writes + barrier, [3] epilogue. */
int bbbp_conv_b3_phases(unsigned long long* phases4);
int bbbp_conv3x3_relu_pool_fwd(void* stream, const float* x, const float* w, const float* bias,
                               float* y, uint8_t* mask, int B, int cin, int cout, int H, int W,
                               void* workspace, size_t workspace_bytes);
int bbbp_conv3x3_relu_pool_bwd_data(void* stream, const float* gy, const uint8_t* mask, const float* w,
                                    float* dx, int B, int cin, int cout, int H, int W,
                                    void* workspace, size_t workspace_bytes);
int bbbp_conv3x3_relu_pool_bwd_weight(void* stream, const float* x, const float* gy, const uint8_t* mask,
                                      float* dw, float* db, int B, int cin, int cout, int H, int W,
                                      void* workspace, size_t workspace_bytes);

/* ---- LayerNorm(x_dropped + residual): nn.TransformerEncoderLayer.norm1/norm2 (R:75-78) ---------
 * forward overwrites x with z = dropout(x) + residual (kept for backward) and writes y, mean, rstd.
 * backward: dz (gradient of the residual input), dx (optional; dz times the dropout keep-scale). */
int bbbp_layernorm_fwd(void* stream, float* x_inout_z, const float* residual, float* y, const float* gamma,
                       const float* beta, float* mean, float* rstd, int rows, int cols, float eps,
                       float dropout_p, uint64_t seed);
/* Linear + dropout + residual + LayerNorm as ONE launch for narrow outputs (the encoder's out_proj -> norm1 and linear2 -> norm2 at
 * F = 167, R:75-78): z = dropout(x W^T + bias) + residual (written, kept for backward), y = LayerNorm(z), mean / rstd per row.  The
 * dropout draws the elements bbbp_layernorm_fwd draws.  bbbp_linear_layernorm_supported: N <= 256, K <= 8192.  The engine uses it for
 * out_proj -> norm1 only with BBBP_FUSED_LINEAR_LN=1 in the environment (measured slower inside the B = 512 step). */
int bbbp_linear_layernorm_supported(int M, int N, int K);
int bbbp_linear_layernorm_fwd(void* stream, const float* x, int ldx, const float* W, const float* bias, const float* residual, int ldr,
                              float* z, int ldz, float* y, int ldy, const float* gamma, const float* beta, float* mean, float* rstd,
                              int M, int N, int K, float eps, float dropout_p, uint64_t seed);
/* LayerNorm ABSORBED by the Linear that consumes it (round 4; the encoder's norm1 -> linear1, norm2 -> the next in_proj / fingerprint_fc,
 * R:75-82): ONE launch computes out = dropout(act(LayerNorm(z) W^T + bias)) [M][N] and writes y = LayerNorm(z) [M][K], mean, rstd (what
 * bbbp_layernorm_fwd writes for a z that already holds dropout(x) + residual -- the producing GEMM's epilogue does that now).  Per output
 * element out = rstd_m (sum_k (z - x0_m) gamma_k W[n][k] - (mu_m - x0_m) c_n) + d_n + bias_n with c_n = sum_k gamma_k W[n][k],
 * d_n = sum_k beta_k W[n][k], all taken from the product's own operand stream (csrc/gemm.hip: gemm_direct_lna_kernel); y / mean / rstd come
 * from one extra column of work-groups of the same launch.  K <= 192 (bbbp_layernorm_linear_supported).  The dropout draws element
 * m * N + n of `seed`, the stream bbbp_dropout draws for a contiguous [M][N] tensor. */
int bbbp_layernorm_linear_supported(int M, int N, int K);
int bbbp_layernorm_linear_fwd(void* stream, const float* z, int ldz, const float* gamma, const float* beta, float eps,
                              const float* W, const float* bias, float* out, int ldo, int act, float dropout_p, uint64_t seed,
                              float* y, int ldy, float* mean, float* rstd, int M, int N, int K);
int bbbp_layernorm_bwd(void* stream, const float* dy, const float* z, const float* gamma, const float* mean,
                       const float* rstd, float* dz, float* dx, float* dgamma, float* dbeta, int rows, int cols,
                       float dropout_p, uint64_t seed);

/* ---- row softmax (attention probabilities, R:75-78 via F.scaled_dot_product_attention) --------- */
int bbbp_softmax_fwd(void* stream, float* x_inout, float* dropped_out, long rows, int cols, float dropout_p,
                     uint64_t seed);
int bbbp_softmax_bwd(void* stream, float* dprob_inout, const float* prob, long rows, int cols, float dropout_p,
                     uint64_t seed);

/* ---- nn.Dropout: y = x * keep-scale; the same call with the same seed is its backward ---------- */
int bbbp_dropout(void* stream, const float* x, float* y, long n, float p, uint64_t seed);

/* ---- nn.BatchNorm1d (R:101): batch statistics + running-stat update when training ------------- */
int bbbp_batchnorm1d_fwd(void* stream, const float* x, float* y, const float* gamma, const float* beta,
                         float* running_mean, float* running_var, float* save_mean, float* save_rstd, int rows,
                         int cols, float eps, float momentum, int training);
int bbbp_batchnorm1d_bwd(void* stream, const float* dy, const float* x, const float* gamma, const float* save_mean,
                         const float* save_rstd, float* dx, float* dgamma, float* dbeta, int rows, int cols,
                         int training);
/* ... followed by the backward of the ReLU that produced x (fc.1 -> fc.2 of the head, R:99-100): dx = 0 where x <= 0 */
int bbbp_batchnorm1d_bwd_relu(void* stream, const float* dy, const float* x, const float* gamma, const float* save_mean,
                         const float* save_rstd, float* dx, float* dgamma, float* dbeta, int rows, int cols,
                         int training);

/* Pieces for a BatchNorm1d whose batch is sharded over ranks (exact-global-batch data parallelism): local column sums of
 * (x - centre) and (x - centre)^2, and dx from sums taken over the global batch of n_global rows. */
int bbbp_column_moments(void* stream, const float* x, const float* centre, float* sum_out, float* sumsq_out, int rows, int cols);
int bbbp_batchnorm1d_bwd_apply(void* stream, const float* dy, const float* x, const float* gamma, const float* mean,
                               const float* rstd, const float* sum_dy, const float* sum_dy_xhat, float* dx, int rows,
                               int cols, long n_global);

/* ---- backward of "+ bias, activation": dy *= act'(y) * scale in place, dbias = column sums ------ */
int bbbp_bias_act_bwd(void* stream, float* dy_inout, int lddy, const float* y, int ldy, float* dbias, int rows,
                      int cols, int act, float scale);

/* ---- MultiHeadAttentionFusion.forward combine step (R:60-65) and its backward ------------------ */
int bbbp_fusion_combine_fwd(void* stream, const float* combined, const float* hid, const float* const* w2,
                            const float* const* b2, float* out, float* attn, int rows, int dim, int hidden,
                            int num_heads);
int bbbp_fusion_combine_bwd(void* stream, const float* dout, const float* combined, const float* hid,
                            const float* attn, const float* const* w2, float* dcombined, float* dlogit,
                            float* dpre, int rows, int dim, int hidden, int num_heads);

/* ---- the fusion block and the regression head as two ops (csrc/head.hip; R:60-65, 98-107): the kernels bbbp_mixed_forward / _backward
 * run between the join of the branches and the loss, with every tensor they read or write an argument.
 * Forward: combined [B][256] -> 4 x (Linear(256,128) -> Tanh -> Linear(128,1)) -> softmax over the heads -> fused = sum_h a_h combined ->
 * h = ReLU(fc.0) -> hb = BatchNorm1d (eps 1e-5, momentum 0.1; training: batch statistics, running statistics updated in place with the
 * unbiased variance; else the running statistics) -> h2 = ReLU(fc.3) -> h3 = ReLU(fc.5) -> out [B] = fc.7.  fw1 / fb1 / fw2 / fb2: host
 * arrays of four device pointers ([128][256], [128], [128], [1] per head); Linear weights are [out][in] and need only 4-byte alignment.
 * Written: hid [4][B][128], attn [B][4], fused [B][256], h, hb [B][256], bn_mean, bn_rstd [256] (the statistics hb was normalised with),
 * h2 [B][128], h3 [B][64], out.  concat != 0: fused IS combined (torch.cat fusion); the fusion block's parameters, hid, attn and fused are
 * neither read nor written and may be NULL.
 * Backward: the input-gradient chain from dout [B] over SAVED tensors taken as given (nothing is recomputed from combined): dh3, dh2, dhb,
 * dh, dlogit [4][B], dpre [4][B][128], dcomb [B][256] (zero where combined <= 0) and the BatchNorm's dgamma, dbeta [256]; training = 0:
 * dh = dhb gamma rstd.  No concat form: the engine runs the per-op chain there.
 * world / rank: the batch is sharded over `world` ranks of B rows EACH (the merge derives every rank's block sizes from this rank's B), and
 * statistics and backward sums are merged over all ranks' 16-row blocks in rank order; dgamma / dbeta stay this rank's sums.  The first
 * launch of a direction writes this rank's slot of `partial`, the second reads every slot: the caller makes the other ranks' slots arrive
 * in between (world = 1, rank = 0: the single-rank head, nothing to do).  `partial`: world * ceil(B / 16) * 2 * 256 floats.
 * BBBP_ERR_ARG before any launch: a NULL required pointer, B < 1, rank outside [0, world), training with B * world <= 1. */
int bbbp_head_fwd(void* stream, const float* comb, const float* const* fw1, const float* const* fb1, const float* const* fw2,
                  const float* const* fb2, const float* w0, const float* b0, const float* gamma, const float* beta,
                  float* running_mean, float* running_var, const float* w3, const float* b3, const float* w5, const float* b5,
                  const float* w7, const float* b7, float* hid, float* attn, float* fused, float* h, float* hb, float* bn_mean,
                  float* bn_rstd, float* h2, float* h3, float* out, float* partial, int B, int training, int concat, int world, int rank);
int bbbp_head_bwd(void* stream, const float* dout, const float* comb, const float* hid, const float* attn, const float* h,
                  const float* h2, const float* h3, const float* bn_mean, const float* bn_rstd, const float* gamma,
                  const float* const* fw1, const float* const* fw2, const float* w0, const float* w3, const float* w5,
                  const float* w7, float* dh3, float* dh2, float* dhb, float* dh, float* dlogit, float* dpre, float* dcomb,
                  float* dgamma, float* dbeta, float* partial, int B, int training, int world, int rank);

/* ---- nn.MSELoss (R:143,189) and its gradient; optim.AdamW.step (R:172,191) -------------------- */
int bbbp_mse(void* stream, const float* pred, const float* target, float* loss, float* dpred, int n, float grad_scale);
/* AdamW: the hyper-parameters are DOUBLES, as torch.optim.AdamW holds them (Python floats): the step's float32 constants are derived in
 * double the way torch derives them and rounded once, and the kernel executes torch's float32 op sequence with every rounding pinned --
 * the moments are torch's bits, the parameters torch's bits on > 99 % of the elements (tests/test_gpu_round4.py). */
int bbbp_adamw_step(void* stream, float* param, const float* grad, float* exp_avg, float* exp_avg_sq, long n,
                    double lr, double beta1, double beta2, double eps, double weight_decay, int step, double grad_scale);
/* The same step with the slice [lo, hi) of the flat buffers updated on a library-owned side stream (round 4).  Everything else is updated on
 * `stream`; the slice starts once the gradients are final (an event on `stream`) and runs beside whatever `stream` does next.  Readers are
 * ordered behind it by the library: bbbp_mixed_forward waits right before its first read of a tensor inside the slice (the image-FC weight:
 * 62 % of the optimizer's bytes, first read 0.8 ms into the next forward pass), every other entry point that reads parameters
 * (bbbp_adamw_step*, bbbp_mixed_backward) waits at its start, and bbbp_param_sync(stream) orders ANY stream behind it (call it before
 * reading parameters outside this library: state_dict(), checkpoints).  Element-wise arithmetic: the result is bit-identical to
 * bbbp_adamw_step's.  Inside a stream capture, or with an empty slice, it IS bbbp_adamw_step. */
int bbbp_adamw_step_deferred(void* stream, float* param, const float* grad, float* exp_avg, float* exp_avg_sq, long n, long lo, long hi,
                             double lr, double beta1, double beta2, double eps, double weight_decay, int step, double grad_scale);
/* Multi-tensor form (round 4): parameters and moments are ONE flat buffer of n elements, the gradients are n_tensors separate device tensors
 * (what autograd leaves behind for a per-op model: torch.optim.AdamW's foreach path, here one launch).  `table_dev`: device memory owned by the
 * caller and read on `stream` -- long offsets[n_tensors + 1] (element offsets into the flat buffer, offsets[0] = 0, offsets[n_tensors] = n)
 * followed by const float* grads[n_tensors].  `hyper_dev` (nullable): eight floats in device memory as bbbp_adamw_hyper_store writes them; then
 * lr ... grad_scale are ignored -- a step captured into a HIP graph replays with whatever the caller stored there before the launch.
 * Same per-element expressions as bbbp_adamw_step: bit-identical to n_tensors single launches. */
int bbbp_adamw_step_multi(void* stream, float* param, float* exp_avg, float* exp_avg_sq, long n, const void* table_dev, int n_tensors,
                          double lr, double beta1, double beta2, double eps, double weight_decay, int step, double grad_scale, const float* hyper_dev);
/* stores those eight floats (derived on the host in double, as bbbp_adamw_step derives them) to device memory in stream order */
int bbbp_adamw_hyper_store(void* stream, float* hyper_dev, double lr, double beta1, double beta2, double eps, double weight_decay, int step, double grad_scale);
/* The structured-sparse weight gradient of the 32->64 / 64->128 / 128->256 stages has an 8-wave form (fastest alone) and a 4-wave form (one
 * wave per SIMD: faster when another branch's small kernels share the GPU).  bbbp_mixed_backward chooses by itself; a caller composing the
 * model op by op with its branches on two streams sets this for the CALLING THREAD around bbbp_conv3x3_relu_pool_bwd_weight.  Returns the
 * previous setting. */
int bbbp_set_conv_wgrad_beside_encoder(int on);
/* Forward of the 32->64 / 64->128 stages on 64 x 64 maps: 1 selects, for the CALLING THREAD, the software-pipelined kernel that runs one
 * work-group per CU (slower alone, faster for a step whose encoder chain runs beside it; bbbp_mixed_forward chooses by itself).  Outputs and
 * decisions are bit-identical.  Returns the previous setting. */
int bbbp_set_conv2_fwd_pipe(int on);
/* Op-level dropout streams keyed from device memory (round 4).  With a base set for the CALLING THREAD, every seeded entry point of this
 * header (dropout, softmax, layernorm, linear with output dropout, attention) uses the stream  *base * 0x9E3779B97F4A7C15 + seed  instead of
 * `seed`: a training step captured into a HIP graph draws new masks on each replay when the caller bumps the 64-bit integer at `base_dev`
 * before it.  NULL restores the default.  Forward and backward of one step must see the same base and the same *base. */
int bbbp_set_seed_base(const void* base_dev);
int bbbp_param_sync(void* stream);
void* bbbp_param_stream(void);     /* the side stream of the current device (NULL before the first deferred step) */
int bbbp_scale(void* stream, float* x, long n, float s);

/* ---- input pipeline at the tensor boundary (Descriptors/multi_input_data_preprocess_maccs_opt_IsolationForest_fixed_1.py) ----
 * :56-71  PIL convert('RGB') + torchvision Resize((128,128)) + ToTensor: Pillow's fixed-point two-pass bilinear
 *         resampling, bit-exact; coefficient tables (bounds [out][2] = {first, count}, kk [out][ksize] int32) come from
 *         the host (preprocess.py: pil_resample_coeffs).  src [N][Hs][Ws][3] u8; tmp [N][Hs][Wo][3] u8 scratch;
 *         dst_u8 [N][Ho][Wo][3] (optional); dst_chw [N][3][Ho][Wo] f32 = byte / 255.
 * :86-101 StandardScaler().fit_transform over one chunk of rows of hstack([fingerprint u8, image f32]), float64
 *         statistics, float32 output; mean_out / scale_out [F+I] optional. */
int bbbp_resize_bilinear_totensor(void* stream, const uint8_t* src, uint8_t* tmp, uint8_t* dst_u8, float* dst_chw,
                                  const int* bounds_x, const int* kk_x, int ksize_x, const int* bounds_y,
                                  const int* kk_y, int ksize_y, int N, int Hs, int Ws, int Ho, int Wo);
int bbbp_standardize_chunk(void* stream, const uint8_t* fingerprint_u8, const float* image, float* fingerprint_out,
                           float* image_out, double* mean_out, double* scale_out, int rows, int F, int I);

/* ---- whole-model entry points: MixedInputModel.forward (R:109-119) and its autograd ------------
 * params[]: device pointers in the reference's named_parameters() order:
 *   per encoder layer l (12): self_attn.in_proj_weight, in_proj_bias, out_proj.weight, out_proj.bias,
 *        linear1.weight, linear1.bias, linear2.weight, linear2.bias, norm1.weight, norm1.bias, norm2.weight, norm2.bias
 *   fingerprint_fc.0.{weight,bias}; image_cnn.{0,3,7}.{weight,bias};
 *   attention_fusion.attention_heads.h.{0.weight,0.bias,2.weight,2.bias} for h in 0..3;
 *   fc.0.{w,b}, fc.2.{w,b} (BatchNorm affine), fc.3.{w,b}, fc.5.{w,b}, fc.7.{w,b}
 * num_layers = 0 drops the encoder (fingerprint_fc reads the fingerprint itself): with fusion = 1 that is BASELINE
 * config 2, the two-branch MACCS-Linear + image-CNN + concat + BatchNorm-head model.
 * grads[]: same order, written (not accumulated).  bn_running: {running_mean, running_var} of fc.2.
 * The workspace carries the saved activations from forward to backward. */
/* Collective hook of the exact-global-batch mode.  Called on the HOST while bbbp_mixed_forward / _backward enqueue their work; the
 * callee must enqueue the collective so that it is ordered after everything enqueued on `stream` so far and before anything enqueued on
 * it later (e.g. torch.distributed under torch.cuda.stream(ExternalStream(stream))).  Buffers are byte offsets into the call's
 * workspace; `count` is in floats PER RANK.  Return 0 on success.
 *   BBBP_COLL_ALLGATHER        recv_off: [world][count] floats, this rank's slot (= send_off) already filled: all-gather in place
 *   BBBP_COLL_REDUCE_SCATTER   send_off: [world][count] floats; recv_off: [count] floats = sum over ranks of their slot `rank`
 * `what`: BBBP_COLL_KV / _DKV (layer = encoder layer) or BBBP_COLL_BN_FWD / _BN_BWD (layer = -1). */
enum { BBBP_COLL_ALLGATHER = 0, BBBP_COLL_REDUCE_SCATTER = 1 };
enum { BBBP_COLL_KV = 0, BBBP_COLL_DKV = 1, BBBP_COLL_BN_FWD = 2, BBBP_COLL_BN_BWD = 3 };
typedef int (*bbbp_collective_fn)(void* ctx, int op, int what, int layer, size_t send_off, size_t recv_off, size_t count, void* stream);

typedef struct {
    int batch;            /* B (also the attention sequence length: R:110-111, batch_first=False) */
    int fingerprint_size; /* F = d_model */
    int nhead;            /* R:71-73 */
    int num_layers;       /* 6 */
    int dim_feedforward;  /* 2048 */
    int training;         /* BatchNorm batch statistics + dropout */
    float dropout_p;      /* 0.1 in the encoder when training */
    uint64_t seed;        /* dropout stream of this step */
    int need_input_grad;  /* unused by the reference (inputs do not require grad) */
    int fusion;           /* 0: MultiHeadAttentionFusion(256, 4 heads) (R:48-65); 1: plain torch.cat of the two branch outputs
                             (Descriptors/multi_input_data_regression_opt_round_2_transformer_cnn.py:99) -- the 16
                             attention_fusion.* entries are then absent from params[] / grads[] */
    int inference;        /* 1: forward only (torch.no_grad()): the workspace omits every backward temporary and the encoder
                             layers share one set of activation buffers; bbbp_mixed_backward refuses such a workspace */
    /* Exact-global-batch data parallelism (SURVEY 8e mode 2; round 3): `batch` is THIS rank's shard of a mini-batch of world * batch
     * molecules.  The two places where the reference couples the molecules of a mini-batch are made global through `collective`:
     * every encoder layer attends over the keys / values of all ranks (the engine packs K | V of its rows into its slot of a
     * [world][batch][2F] buffer and asks for an in-place all-gather; backward, its queries' share of dK | dV for ALL keys is
     * reduce-scattered), and the head's BatchNorm1d merges the per-16-row (mean, M2) blocks / backward sums of all ranks (all-gather of
     * [blocks][2][256] floats).  With gradients averaged over ranks an N-rank step equals the single-GPU step at world * batch.
     * collective == NULL (and world <= 1): the replica engine, nothing changes. */
    int world;            /* ranks sharing the mini-batch (0 / 1 with a callback: the same code path with no-op collectives) */
    int rank;             /* this rank's position: its rows are global rows rank * batch .. */
    bbbp_collective_fn collective;
    void* collective_ctx;
} bbbp_mixed_desc;

int bbbp_mixed_num_params(const bbbp_mixed_desc* d);
size_t bbbp_mixed_workspace_bytes(const bbbp_mixed_desc* d);
int bbbp_mixed_forward(void* stream, const bbbp_mixed_desc* d, const float* const* params, float* const* bn_running,
                       const float* fingerprint, const float* image, float* out, void* workspace, size_t workspace_bytes);
int bbbp_mixed_backward(void* stream, const bbbp_mixed_desc* d, const float* const* params, float* const* grads,
                        const float* fingerprint, const float* image, const float* dout, void* workspace,
                        size_t workspace_bytes);

/* ---- batched trainer for scikit-learn style MLP classifiers (Models/model_opt_maccs.py:133,170-181: MLPClassifier under
 * GridSearchCV).  One persistent work-group trains one model; float64, scikit-learn's
 * arithmetic (binary log-loss + L2, Adam, training-loss stopping rule).  The array of models lives in DEVICE memory; the
 * host fills it (including the device pointers), supplies `order` = the global row ids of each of the next `epochs`
 * epochs in visiting order, launches, and reads back n_iter / done / loss_curve.  parameter layout: [W0|b0|W1|b1|...],
 * W[l] is [units[l]][units[l+1]] row-major (scikit-learn's coefs_). */
typedef struct bbbp_mlp_model {
    int n_layers;                 /* weight layers: hidden layers + 1 (2 or 3 for the reference grid; at most 4) */
    int units[5];                 /* units[0] = n_features ... units[n_layers] = 1 */
    int activation;               /* hidden activation: 0 relu, 1 tanh */
    int batch_size;
    int n_train;                  /* rows visited per epoch */
    int n_iter_no_change, max_iter;
    double lr_init, alpha, beta1, beta2, eps, tol;
    double* params; double* adam_m; double* adam_v; double* grads;
    double* act; double* delta;   /* scratch: batch_size * (sum of units[1..n_layers]) each */
    const int* order;             /* [epochs][n_train] */
    double* loss_curve;           /* [max_iter] */
    long t;                       /* Adam step count */
    double best_loss;             /* +inf at start */
    int no_improve, n_iter, done;
} bbbp_mlp_model;
int bbbp_mlp_train_epochs(void* stream, bbbp_mlp_model* models_dev, int n_models, const double* X, const double* y,
                          int n_features, int epochs);
/* out[i] = P(class 1 | X[i]) under models_dev[model]; hidden layers up to 256 units */
int bbbp_mlp_predict_proba(void* stream, const bbbp_mlp_model* models_dev, int model, const double* X, int n, int n_features,
                           int max_units, double* out);
/* Phase profile of the trainer's persistent kernel: on != 0 selects an instrumented build of the kernel for later bbbp_mlp_train_epochs calls
 * (work-group 0 adds the shader-clock cycles of each phase of every mini-batch to 16 counters) and clears them; cycles16 (host, nullable) gets
 * the counters accumulated so far: 0-2 forward layer l, 3 loss, 4 + 2 l / 5 + 2 l delta / weight gradient + Adam of layer l, 10 mini-batch
 * tail, 11 epoch tail, 15 mini-batches. */
int bbbp_mlp_profile(int on, unsigned long long* cycles16);
/* ... and per work-group (= per fit, in device-array order) of the last instrumented launch: out[3 g] / out[3 g + 1] = 100 MHz wall ticks at its
 * start / end, out[3 g + 2] = shader cycles in between (who finishes last, and at which clock) */
int bbbp_mlp_profile_groups(unsigned long long* out, int n_groups);

/* ---- random-forest regression inference (rf base learner of the stack, ...20250113.py:262-266, 394-403) -------------
 * scikit-learn's semantics: float32 X, go left when (double)x[feature] <= threshold, leaf value in float64, mean over
 * trees in float64.  Node arrays are the trees' arrays concatenated (child indices rebased), root[t] = first node of
 * tree t (n_trees + 1 entries); partial: bbbp_forest_groups(n_trees) * n doubles of scratch. */
int bbbp_forest_groups(int n_trees);
int bbbp_forest_predict(void* stream, const float* X, long n, int n_features, const int* left, const int* right,
                        const int* feature, const double* threshold, const double* value, const int* root, int n_trees,
                        double* partial, double* out);

/* ---- gradient-boosted regression trees, prediction (the xgb base learner of the stack, ...20250108.py:186-189; fitted model
 * Models/xgb_model_maccs.pkl) -- XGBoost's predict rule: left when x[feature] < split_condition (float32), the default child when
 * the feature is NaN, leaf value in split_condition[leaf], out = base_score + float32 sum of the leaves in tree order.  Node arrays
 * concatenated over trees (child indices rebased, -1 = leaf), root[t] = first node of tree t; leaf_scratch: n_trees * n floats.
 * The caller validates the arrays (boosters.validate_gbt: children inside their tree, one parent per node, split indices below
 * n_features); the device walk stops after 1024 levels all the same and then yields NaN for that (tree, row). */
int bbbp_gbt_predict(void* stream, const float* X, long n, int n_features, const int* left, const int* right, const int* feature,
                     const float* split_condition, const uint8_t* default_left, const int* root, int n_trees, float base_score,
                     float* leaf_scratch, float* out);

/* ---- oblivious (symmetric) trees, prediction (the cat base learner of the stack, ...20250108.py:192-195) -- CatBoost's rule for float
 * features: bit i of a tree's leaf index is x[split_feature] > split_border of its level i (NaN: false, or true where nan_true[feature]),
 * out = scale * (float64 sum of leaf_values[tree_first_leaf[t] + index] in tree order) + bias.  Splits concatenated over trees
 * (tree_first_split: n_trees + 1 entries, at most 31 levels per tree); leaf_scratch: n_trees * n doubles. */
int bbbp_oblivious_predict(void* stream, const float* X, long n, int n_features, const int* split_feature, const float* split_border,
                           const uint8_t* nan_true, const int* tree_first_split, const long* tree_first_leaf, const double* leaf_values,
                           int n_trees, double scale, double bias, double* leaf_scratch, double* out);

/* ---- staged prediction of both boosted families (the per-iteration curves of ...20250113.py:289-391 and the truncated model of
 * use_best_model=True, from one walk of the trees).  Stage k = 0 .. K - 1 covers the trees [tree_start, e_k), e_k = min(tree_start +
 * (k + 1) * period, tree_end); K = bbbp_staged_count(tree_start, tree_end, period) = ceil((tree_end - tree_start) / period), 0 for a bad
 * range or period.  out[k * ldo + i] holds, bit for bit, what bbbp_gbt_predict / bbbp_oblivious_predict return for row i and a model of
 * the trees [tree_start, e_k) alone (float32 / float64, summed in ascending tree order, the offset last).  The model arrays are the whole
 * model's, as for the predict entry points; 0 <= tree_start < tree_end <= n_trees, period >= 1, ldo >= n (a caller that works in row
 * chunks passes the full row count as ldo and out + its first row).  leaf_scratch: (tree_end - tree_start) * n floats / doubles.  Two
 * launches whatever K is; nothing of out or leaf_scratch is read before it is written, out[k][n .. ldo) is not touched. */
int bbbp_staged_count(int tree_start, int tree_end, int period);
int bbbp_gbt_staged_predict(void* stream, const float* X, long n, int n_features, const int* left, const int* right, const int* feature,
                            const float* split_condition, const uint8_t* default_left, const int* root, int n_trees, float base_score,
                            int tree_start, int tree_end, int period, float* leaf_scratch, float* out, long ldo);
int bbbp_oblivious_staged_predict(void* stream, const float* X, long n, int n_features, const int* split_feature, const float* split_border,
                                  const uint8_t* nan_true, const int* tree_first_split, const long* tree_first_leaf,
                                  const double* leaf_values, int n_trees, double scale, double bias, int tree_start, int tree_end, int period,
                                  double* leaf_scratch, double* out, long ldo);

/* ---- PCA: float64 column means and centred products on the float64 matrix pipe (csrc/pca.hip) -----------------------
 * sklearn.decomposition.PCA(n).fit_transform in front of the PCA-fusion models (Models/multi_input_data_regression_opt_transformer_cnn_opt.py:30-33,
 * its _morgan / _rdkit / _opt_more siblings) and of the MLPClassifier grid (Models/model_opt_maccs.py:104-109).  bbbp_amd/decomposition.py
 * composes a fit from these and a host eigen-solve of the min(n, d)^2 matrix. */
#define BBBP_DTYPE_F32 0
#define BBBP_DTYPE_F64 1
#define BBBP_F64C_NT 0   /* both operands k-contiguous: A[m * lda + k], B[n * ldb + k] */
#define BBBP_F64C_TN 1   /* both operands k-major:      A[k * lda + m], B[k * ldb + n] */
/* mean[j] = (sum_i X[i * ld + j]) / n in float64, X float32 or float64 (dtype: BBBP_DTYPE_*).  Fixed summation order: two calls give the
 * same bits.  A non-finite input yields a non-finite mean. */
int bbbp_pca_col_mean(void* stream, const void* X, int dtype, long n, int d, long ld, double* mean);
/* C[M,N] = row_scale[m] * sum_k (A(m,k) - sa) (B(n,k) - sb), accumulated in float64.  The shifts are subtracted per element in float64
 * while the operand is staged (never algebraically): a_shift / b_shift are indexed by k in NT (length K) and by the operand's own row /
 * column index in TN (length M / N); NULL = no shift.  C is float64, or float32 rounded once from the accumulator.
 * symmetric != 0: B must be A (same pointer, leading dimension, dtype, shift), M == N, no row_scale; only tiles on or below the diagonal are
 * computed and every element is written to (m, n) and (n, m): C is bitwise symmetric.
 * split_k: 0 lets the plan choose the number of K slabs, > 0 forces it.  With more than one slab the partial products go to `workspace`
 * (bbbp_gemm_f64c_workspace_bytes for the same descriptor) and a second launch adds them in slab order: results are bit-reproducible. */
typedef struct bbbp_gemm_f64c_desc {
    int layout;                   /* BBBP_F64C_NT / BBBP_F64C_TN */
    int M, N, K;
    const void* A; int a_dtype; long lda;
    const void* B; int b_dtype; long ldb;
    const double* a_shift; const double* b_shift;
    const double* row_scale;      /* [M], nullable */
    void* C; int c_dtype; long ldc;
    int symmetric;
    int split_k;
} bbbp_gemm_f64c_desc;
/* 0 with a message in bbbp_last_error() for an invalid descriptor (pointers are not examined); 0 also when one slab suffices */
size_t bbbp_gemm_f64c_workspace_bytes(const bbbp_gemm_f64c_desc* d);
int bbbp_gemm_f64c(void* stream, const bbbp_gemm_f64c_desc* d, void* workspace, size_t workspace_bytes);

/* ---- neighbors: fused float64 brute-force k-nearest-neighbour search and classifier vote (csrc/knn.hip) ------------------
 * KNeighborsClassifier() of the classification stack (Models/model_opt_maccs.py:126, 143-144) and the neighbour query a SMOTE starts
 * with.  Euclidean metric, k <= 32.  The [m][n] distance matrix never exists in memory: HBM traffic is the operands, the norms and the
 * lists.  bbbp_amd/neighbors.py composes NearestNeighbors / KNeighborsClassifier / grid_search_cv from these. */
#define BBBP_KNN_UNIFORM 0
#define BBBP_KNN_DISTANCE 1
/* norms[i] = sum_k (X[i * ld + k] - mu[k])^2 in float64 (mu NULL: no shift), fixed summation order.  ORs 1 into *nonfinite (a device
 * word the caller zeroed) when a row's sum is NaN or infinite -- a NaN / infinite element, or an overflowing square. */
int bbbp_knn_row_norms(void* stream, const void* X, int dtype, long n, int d, long ld, const double* mu, double* norms, int* nonfinite);
/* For every query row the k training rows of smallest Euclidean distance, in the total order (distance, training index).
 * Selection runs on s = |q - mu|^2 + |t - mu|^2 - 2 (q - mu).(t - mu) with the Gram term on the float64 matrix pipe and the shift subtracted
 * at staging; q_norm / t_norm are bbbp_knn_row_norms of Q / T with the same mu.  The k kept rows then get their distance recomputed by
 * direct differences and are sorted again: dist is sqrt of that (exactly 0 for a duplicate of the query), ind the training index.
 * exclude_self != 0: Q must be T (same pointer, leading dimension, dtype, m == n) and row i is not a neighbour of query i.
 * slices: 0 lets the plan choose how many slices the training rows are cut into, > 0 forces it (<= 64).  With more than one slice the
 * partial lists go to `workspace` (bbbp_knn_workspace_bytes for the same descriptor) and a merge launch combines them; the result is
 * bit-identical for every slice count and from call to call. */
typedef struct bbbp_knn_desc {
    int m, n, d, k;
    const void* Q; int q_dtype; long ldq;      /* [m][d], BBBP_DTYPE_* */
    const void* T; int t_dtype; long ldt;      /* [n][d] */
    const double* mu;                          /* [d], nullable */
    const double* q_norm; const double* t_norm;
    double* dist; long long* ind;              /* [m][k] each */
    int exclude_self;
    int slices;
} bbbp_knn_desc;
/* 0 with a message in bbbp_last_error() for an invalid descriptor (pointers are not examined); 0 also when one slice suffices */
size_t bbbp_knn_workspace_bytes(const bbbp_knn_desc* d);
int bbbp_knn_f64(void* stream, const bbbp_knn_desc* d, void* workspace, size_t workspace_bytes);
/* Class vote over the first kk of the k neighbours of each of m queries.  labels[n]: class id (0 .. n_classes - 1, n_classes <= 32) of
 * every training row.  weights: BBBP_KNN_UNIFORM, or BBBP_KNN_DISTANCE = 1 / dist, where a query with a zero among its kk distances
 * gives those neighbours weight 1 and the others 0.  Weights are added in neighbour order in float64.  proba[m][n_classes] is
 * normalised; pred[m] is the class of largest weight, the lowest id on ties. */
int bbbp_knn_vote(void* stream, const double* dist, const long long* ind, long m, int k, int kk, const int* labels, long n, int n_classes,
                  int weights, double* proba, int* pred);

/* ---- svm: float64 kernel matrix, batched SMO solver and fused decision function (csrc/svm.hip) ---------------------------
 * SVC() of the classification stack (Models/model_opt_maccs.py:124-180), searched over C in {0.1, 1, 10} x kernel in {linear, rbf}.
 * bbbp_amd/svm.py composes SVC / grid_search_cv from these. */
#define BBBP_SVM_LINEAR 0
#define BBBP_SVM_RBF 1
/* K[i][j] = sum_k X[i][k] X[j][k] (linear, uncentred: mu and norms are not read) or exp(-gamma |x_i - x_j|^2) (rbf), float64.
 * rbf: the squared distance is |x_i - mu|^2 + |x_j - mu|^2 - 2 (x_i - mu).(x_j - mu), clamped at 0, with the inner product on the float64
 * matrix pipe, the shift subtracted at staging and norms = the row-norm entry point of the neighbours section run on X with the same mu
 * (which also flags non-finite input).  K is bitwise symmetric and the rbf diagonal is exactly 1. */
typedef struct bbbp_svm_kernel_desc {
    int n, d;
    int kernel;                                /* BBBP_SVM_* */
    double gamma;
    const void* X; int x_dtype; long ldx;      /* [n][d], BBBP_DTYPE_* */
    const double* mu;                          /* [d], nullable */
    const double* norms;                       /* [n], rbf only */
    double* K; long ldk;                       /* [n][ldk] */
} bbbp_svm_kernel_desc;
int bbbp_svm_kernel_matrix(void* stream, const bbbp_svm_kernel_desc* d);
/* One C-SVC dual problem: min 1/2 a^T Q a - e^T a, 0 <= a <= C, y^T a = 0, Q[s][t] = y[s] y[t] K[r(s)][r(t)] with r = rows (NULL: the
 * identity), so that a fold is a subset of one shared matrix; every entry of rows must index a row of K.  y holds +1.0 / -1.0.
 * State: alpha and grad (start a problem with alpha = 0, grad = -1, *n_iter = 0, *done = 0); diag is scratch of n doubles.
 * Outputs: *rho, *n_iter (iterations so far), *done (1 once m(alpha) - M(alpha) < tol). */
typedef struct bbbp_svm_problem {
    const double* K; long ldk;
    const int* rows;                           /* [n], nullable */
    const double* y;                           /* [n] */
    double* alpha; double* grad; double* diag; /* [n] each */
    double* rho; int* n_iter; int* done;
    int n;
    double C, tol;
} bbbp_svm_problem;
/* libsvm's solver without shrinking (second-order working-set selection, its clipping, tau = 1e-12, ties to the later index), one
 * work-group per problem.  A launch runs at most `iters` iterations of every problem whose *done is 0 and returns: the caller reads the
 * done flags and calls again with the unfinished problems.  `problems` is a host array.  A problem's result does not depend on the
 * others in the batch and is bit-identical from call to call. */
int bbbp_svm_smo(void* stream, const bbbp_svm_problem* problems, int n_problems, int iters);
/* out[q] = sum_s coef[s] k(SV[s], Q[q]) + intercept, the kernel as above (rbf: q_norm / sv_norm are the row norms of Q / SV with the same mu).
 * The kernel block is consumed in registers; one partial sum per (tile of 64 support vectors, query) goes to `workspace`
 * (bbbp_svm_decision_workspace_bytes for the same descriptor) and a second launch adds them in tile order.  slices: 0 lets the plan choose
 * how many work-groups share a query tile's support vectors, > 0 forces it (<= 64); the result does not depend on it. */
typedef struct bbbp_svm_decision_desc {
    int m, n_sv, d;
    int kernel;
    double gamma;
    const void* Q; int q_dtype; long ldq;      /* [m][d] */
    const void* SV; int sv_dtype; long ldsv;   /* [n_sv][d] */
    const double* mu;                          /* [d], nullable */
    const double* q_norm; const double* sv_norm;
    const double* coef;                        /* [n_sv] */
    double intercept;
    double* out;                               /* [m] */
    int slices;
} bbbp_svm_decision_desc;
/* 0 with a message in bbbp_last_error() for an invalid descriptor (pointers are not examined) */
size_t bbbp_svm_decision_workspace_bytes(const bbbp_svm_decision_desc* d);
int bbbp_svm_decision(void* stream, const bbbp_svm_decision_desc* d, void* workspace, size_t workspace_bytes);
/* One epsilon-SVR dual problem (csrc/svr.hip; SVR(kernel='rbf', C=1.0, epsilon=0.1) of the regression stack,
 * Models/multi_input_data_regression_opt_transformer_cnn_opt_more.py:117-149): 2n variables over the n x n matrix, variable k < n with
 * sign s = +1 and linear term epsilon - t[k], variable k + n with s = -1 and linear term epsilon + t[k];
 * Q[k][l] = s_k s_l K[r(k mod n)][r(l mod n)] with r = rows (NULL: the identity), every entry of rows indexing a row of K.
 * State: alpha and grad hold the 2n variables in that order; the launch that finds *n_iter == 0 sets alpha = 0 and grad = the linear term
 * itself, whatever the arrays hold, so the host initialises only *n_iter = 0 and *done = 0.  diag is scratch of n doubles.
 * Outputs: *rho, *n_iter (iterations so far), *done (1 once m(alpha) - M(alpha) < tol).  The regression coefficient of row k is
 * alpha[k] - alpha[k + n] and the intercept -*rho; the kernel matrix and the decision function are the entry points above. */
typedef struct bbbp_svr_problem {
    const double* K; long ldk;
    const int* rows;                           /* [n], nullable */
    const double* t;                           /* [n] targets */
    double* alpha; double* grad;               /* [2n] each */
    double* diag;                              /* [n] */
    double* rho; int* n_iter; int* done;
    int n;
    double C, epsilon, tol;
} bbbp_svr_problem;
/* libsvm's epsilon-SVR solver without shrinking (second-order working-set selection, its clipping, tau = 1e-12, ties to the later index of
 * the 2n ordering), one work-group per problem, called like the classification solver above: at most `iters` iterations per launch of
 * every problem whose *done is 0.  Up to 4096 rows a launch keeps its state in registers (read once, written once); beyond, in alpha and
 * grad.  A problem's result does not depend on `iters`, on the others in the batch or on their order, and is bit-identical from call to
 * call. */
int bbbp_svr_smo(void* stream, const bbbp_svr_problem* problems, int n_problems, int iters);
/* Class probabilities for the C-SVC above by Platt scaling (csrc/svm_proba.hip; SVC(probability=True) of the classification stack,
 * Models/model_opt_maccs.py:128): out-of-fold decision values read from the resident kernel matrix, libsvm's sigmoid_train (Lin, Lin and
 * Weng, "A note on Platt's probabilistic outputs for support vector machines") and its sigmoid_predict.  Float64 throughout; every result
 * is bit-identical from call to call and does not depend on what else is in the batch.
 *
 * One fold whose dual problem the solver above has finished over the matrix K of n_rows data rows: rows / y / alpha / rho / n are that
 * problem's (rows NULL: the identity; rho stays on the device), held lists the n_held rows of K the fold left out.  For each of them
 * out[held[h]] = sum_s alpha[s] y[s] K[held[h]][rows[s]] - *rho, libsvm's decision value (positive towards y = +1), the terms added by
 * one wavefront: lane l takes s = l, l + 64, ... in ascending order and a butterfly adds the 64 lanes.  Every entry of rows and held must
 * lie in [0, n_rows); an entry outside is skipped (a held row is not written, a training row adds nothing).  n_held may be 0. */
typedef struct bbbp_svm_oof_desc {
    const double* K; long ldk; int n_rows;     /* [n_rows][ldk] */
    const int* rows;                           /* [n], nullable */
    const double* y; const double* alpha;      /* [n] each */
    const double* rho;                         /* [1], device */
    int n;
    const int* held; int n_held;               /* [n_held] */
    double* out;                               /* [n_rows], indexed by data row */
} bbbp_svm_oof_desc;
/* `folds` is a host array; up to 32 folds are one launch. */
int bbbp_svm_oof_decision(void* stream, const bbbp_svm_oof_desc* folds, int n_folds);
/* One calibration problem: min over (A, B) of sum_i t_i f_i + log(1 + exp(-f_i)), f_i = A dec[i] + B, with the targets
 * t_i = (N+ + 1) / (N+ + 2) where y[i] > 0 and 1 / (N- + 2) elsewhere (N+ / N- count the two kinds).  Outputs: ab = (A, B);
 * info = (Newton iterations, status). */
#define BBBP_PLATT_CONVERGED 0          /* both gradient components below 1e-5 */
#define BBBP_PLATT_LINE_SEARCH 1        /* the step fell below 1e-10 without sufficient decrease */
#define BBBP_PLATT_MAX_ITER 2           /* 100 iterations */
typedef struct bbbp_svm_platt_problem {
    const double* dec; const double* y;        /* [n] each */
    int n;
    double* ab;                                /* [2] */
    int* info;                                 /* [2] */
} bbbp_svm_platt_problem;
/* libsvm's sigmoid_train, one work-group per problem and no host round trip inside one: Newton's method from A = 0,
 * B = log((N- + 1) / (N+ + 1)), the Hessian's diagonal raised by 1e-12, backtracking by halves with the Armijo constant 1e-4, the
 * overflow-safe two-branch forms of the objective and of p and q.  The five sums of an iteration and each line-search objective are one pass
 * over dec: per thread its elements in ascending order, the 64 lanes of a wave by a butterfly, the waves in ascending order.  `problems`
 * is a host array. */
int bbbp_svm_platt_fit(void* stream, const bbbp_svm_platt_problem* problems, int n_problems);
/* proba[q][0] = 1 / (1 + exp(A dec[q] + B)) by libsvm's two-branch sigmoid_predict, clipped to [1e-7, 1 - 1e-7];
 * proba[q][1] = 1 - proba[q][0].  m may be 0. */
int bbbp_svm_platt_proba(void* stream, const double* dec, long m, double A, double B, double* proba);

/* ---- logreg: batched float64 Newton solver for binary L2 logistic regression (csrc/logreg.hip) ------------------------------
 * LogisticRegression(max_iter=1000) of the classification stack (Models/model_opt_maccs.py:124-180), searched over C in {0.1, 1, 10}.
 * bbbp_amd/linear_model.py composes LogisticRegression / grid_search_cv from these.
 * Objective (scikit-learn's scaling): f(w, b) = 1/n sum_i log(1 + exp(s_i)) + |w|^2 / (2 C n), s_i = -z_i for t_i = 1 and z_i for t_i = 0,
 * z = X w + b; the intercept is not penalised; a problem is converged once max |grad f| <= tol.  theta = (w[0..d), b) holds d + 1 doubles
 * whether or not the intercept is fitted (b stays 0 without it). */
#define BBBP_LOGREG_MAX_D 255
#define BBBP_LOGREG_RUNNING 0          /* *status while a problem is not done */
#define BBBP_LOGREG_CONVERGED 0        /* *status once done: max |grad f| <= tol */
#define BBBP_LOGREG_MAX_ITER 1         /* max_iter accepted steps taken */
#define BBBP_LOGREG_LINE_SEARCH 2      /* 21 trial steps rejected */
#define BBBP_LOGREG_PIVOT 3            /* a non-positive Cholesky pivot */
typedef struct bbbp_logreg_problem {
    const void* X; int x_dtype; long ld;       /* [n][d], BBBP_DTYPE_* */
    int n, d;
    const double* t;                           /* [n], 0.0 / 1.0 */
    double C, tol;
    int fit_intercept;
    int max_iter;                              /* accepted Newton steps, >= 1 */
    double* theta;                             /* [d + 1]: the last accepted point, the result */
    double* trial;                             /* [d + 1]: the point the next round evaluates */
    double* state;                             /* bbbp_logreg_state_bytes(n, d) bytes of solver state and partial sums */
    int* flags;                                /* [4]: n_iter (accepted steps), status (BBBP_LOGREG_*), done, trials of the current line search */
} bbbp_logreg_problem;
/* Bytes of a problem's `state` (0 with a message for n < 1, d < 1 or d > BBBP_LOGREG_MAX_D).  It depends on n and d only, as does the
 * order of every sum: a problem's numbers do not depend on what else is in the batch. */
size_t bbbp_logreg_state_bytes(int n, int d);
/* Offsets, in doubles, of what a round leaves in `state` for the trial point it evaluated: out[0] the loss f, out[1] the gradient [d + 1],
 * out[2] z [n], out[3] the residual r = p - t [n], out[4] the curvature w [n], out[5] the Hessian's upper triangle packed by rows
 * (row a holds columns a .. p - 1, p = d + fit_intercept; bbbp_logreg_eval only: the solver factors it in place). */
int bbbp_logreg_state_layout(int n, int d, long out[6]);
/* `rounds` rounds of the damped Newton iteration for every problem whose done flag is 0, all problems side by side: (1) the row pass --
 * z, r, w and per-block partial sums of the loss, gradient and the Hessian's intercept row at `trial`; (2) the weighted Gram matrix
 * X^T diag(w) X on the float64 matrix pipe, one triangle, in row slabs; (3) one work-group per problem sums the partials in fixed order,
 * accepts or rejects the trial (scikit-learn's NewtonSolver rules: f' <= f + 2^-11 alpha g.s, or |f' - f| <= 16 eps |f| with a smaller
 * 1-norm of the gradient; at most 21 halvings), tests convergence and max_iter, factors H by Cholesky, solves and writes the next trial.
 * Start a problem with theta, trial, state and flags zeroed.  `problems` is a host array; the caller reads the done flags and calls again
 * while any is 0. */
int bbbp_logreg_rounds(void* stream, const bbbp_logreg_problem* problems, int n_problems, int rounds);
/* One evaluation at `trial` with no step: loss, gradient, z, r, w and the packed Hessian in `state` (bbbp_logreg_state_layout). */
int bbbp_logreg_eval(void* stream, const bbbp_logreg_problem* problem);
/* out[q] = sum_k X[q][k] theta[k] + (fit_intercept ? theta[d] : 0): the row pass's dot product, so a training row's value is bitwise the
 * one the solver saw. */
int bbbp_logreg_decision(void* stream, const void* X, int x_dtype, long ld, int m, int d, const double* theta, int fit_intercept, double* out);

/* ---- gbt fit: gradient-boosted classification trees fitted by exact split search (csrc/gbt.hip) --------------------------------
 * GradientBoostingClassifier of the classification stack (Models/model_opt_maccs.py:124-200): two classes, log-loss, friedman_mse, no
 * subsampling, the prior as init.  bbbp_amd/gradient_boosting.py composes GradientBoostingClassifier / grid_search_cv from these.
 * A chain is one model being fitted; chains over one training matrix share XT and order0.  A tree t of a chain owns the node slots
 * [t * capacity, t * capacity + tree_nodes[t]) of the six node arrays, capacity = 2^(max_depth + 1) - 1; nodes are numbered level by
 * level from the root 0, children are tree-relative, -1 marks a leaf (feature 0, threshold -2 there); value is mean(g) of a split
 * node and the update mean(g) / mean(p (1 - p)) of a leaf. */
#define BBBP_GBT_FIT_MAX_N 8192
#define BBBP_GBT_FIT_MAX_D 1024
#define BBBP_GBT_FIT_MAX_DEPTH 7
#define BBBP_GBT_FIT_MAX_TREES 10000
#define BBBP_GBT_FIT_MAX_WALK 4096        /* steps of one tree walk in the decision kernel; a longer walk yields NaN */
typedef struct bbbp_gbt_chain {
    const float* XT;                           /* [d][n]: the training matrix, float32, one feature after the other */
    const int* order0;                         /* [d][n]: per feature the row indices sorted stably by value */
    const double* y;                           /* [n], 0.0 / 1.0 */
    int n, d;
    int n_estimators, max_depth, min_samples_split, min_samples_leaf;
    double learning_rate;
    double init;                               /* the raw score every row starts from */
    void* work;                                /* bbbp_gbt_fit_work_bytes(n, d) bytes, 16-byte aligned; need not be initialised */
    int* left; int* right; int* feature; int* n_node_samples; double* threshold; double* value;      /* [n_estimators][capacity] */
    int* tree_nodes;                           /* [n_estimators]; -1 from the first tree on in which an index left its array (a defect) */
    double* train_score;                       /* [n_estimators]: scikit-learn's train_score_, 2 x the mean of log(1 + exp(raw)) - y raw after each stage */
    double* raw;                               /* [n]: the training rows' raw scores after the last stage */
} bbbp_gbt_chain;
/* Node slots per tree, 2^(max_depth + 1) - 1 (0 with a message outside 1..BBBP_GBT_FIT_MAX_DEPTH). */
int bbbp_gbt_fit_tree_capacity(int max_depth);
/* Bytes of a chain's `work` (0 with a message for n < 2, d < 1, n > BBBP_GBT_FIT_MAX_N or d > BBBP_GBT_FIT_MAX_D). */
size_t bbbp_gbt_fit_work_bytes(int n, int d);
/* Fit every chain, all side by side, without a host read: max over chains of n_estimators * (max_depth + 1) rounds of six launches.
 * `chains` is a host array, `chains_device` the same bytes in device memory (the kernels read their descriptors there).  A chain's
 * numbers do not depend on what else is in the batch. */
int bbbp_gbt_fit(void* stream, const bbbp_gbt_chain* chains, const bbbp_gbt_chain* chains_device, int n_chains);
/* The same fit under the squared error: GradientBoostingRegressor of the logBB stack's bake-off
 * (Models/multi_input_data_regression_opt_transformer_cnn_opt_more.py:118-125).  Same descriptor, limits, work area and tree capacity;
 * the fields read: y the float64 targets (any finite values), init their mean, value = sum g / m in every node, split node and leaf
 * alike, with g = y - raw (scikit-learn skips the leaf update for this loss: the tree's own node mean is the step), train_score[t] the
 * mean of (y - raw)^2 after stage t.  Messages carry the prefix gbr_fit.  The stats, split, choose, side and partition rules, the tie
 * rule and the determinism are bbbp_gbt_fit's; bbbp_gbt_staged_decision predicts. */
int bbbp_gbr_fit(void* stream, const bbbp_gbt_chain* chains, const bbbp_gbt_chain* chains_device, int n_chains);
/* out[s][q] = init + sum over the first stages[s] trees, in tree order, of learning_rate * value[leaf] (scikit-learn's predict_stages
 * order, product and sum rounded separately) for query rows X [m][d] float32: one pass over the trees.  Children are absolute indices
 * into the node arrays, root[t] is tree t's first node; `stages` (device, [n_stages]) ascends strictly within 1..n_trees; a row goes
 * left when (double)x[feature] <= threshold. */
int bbbp_gbt_staged_decision(void* stream, const float* X, long ld, int m, int d, const int* left, const int* right, const int* feature,
                             const double* threshold, const double* value, const int* root, int n_trees, double init, double learning_rate,
                             const int* stages, int n_stages, double* out);

/* ---- xgb fit: histogram-boosted regression trees, XGBoost's hist updater for reg:squarederror (csrc/xgb.hip) ---------------------
 * XGBRegressor of the logBB stack (Models/multi_input_data_regression_opt_transformer_cnn_20250108.py:186-189).  bbbp_amd/xgb.py states
 * the algorithm and composes XGBRegressor / fit_regressors from these.  A problem is one model being fitted.  Its features are bytes:
 * bins[f][i] = the number of feature f's cuts <= x, cuts[f] padded with +infinity to cut_stride entries.  A tree t owns the node slots
 * [t * capacity, t * capacity + tree_nodes[t]) of the seven node arrays; node ids are XGBoost's (the root 0, nodes expanded level by
 * level in ascending id, each split appends its left and right child as the next two ids), children are tree-relative, -1 marks a leaf;
 * cond is the split's threshold cuts[feature][bin] (a row goes left when x < cond, which is bin <= split bin) or the leaf's value
 * float32((double)learning_rate * w); base_weight is w = -G / (H + lambda) in a split node and the leaf's value in a leaf; loss_change is
 * the gain (0 in a leaf); sum_hessian the row count.  feature counts the columns of `bins`. */
#define BBBP_XGB_FIT_MAX_N 8192
#define BBBP_XGB_FIT_MAX_D 65536
#define BBBP_XGB_FIT_MAX_DEPTH 1024
#define BBBP_XGB_FIT_MAX_TREES 10000
typedef struct bbbp_xgb_problem {
    const uint8_t* bins;                       /* [d][n] */
    const float* cuts;                         /* [d][cut_stride] */
    const float* y;                            /* [n]: the targets rounded to float32 */
    int n, d, cut_stride;
    int n_estimators, max_depth;
    int min_child_rows;                        /* max(1, ceil(min_child_weight)): the hessian of a row is 1 */
    double reg_lambda, gamma;
    float learning_rate, base_score;
    void* work;                                /* bbbp_xgb_fit_work_bytes(n, d) bytes, 16-byte aligned; need not be initialised */
    int* left; int* right; int* feature; float* cond; float* base_weight; float* loss_change; float* sum_hessian;      /* [n_estimators][capacity] */
    int* tree_nodes;                           /* [n_estimators]; -1 from the first tree on in which an index left its array (a defect) */
    float* margin;                             /* [n]: the training rows' margins after the last tree */
} bbbp_xgb_problem;
/* Node slots per tree, min(2 n - 1, 2^(max_depth + 1) - 1) (0 with a message outside the limits above). */
int bbbp_xgb_fit_tree_capacity(int n, int max_depth);
/* Bytes of a problem's `work` (0 with a message outside the limits above). */
size_t bbbp_xgb_fit_work_bytes(int n, int d);
/* bins[f][i] = the number of entries of cuts[f] that are <= XT[f][i], by binary search; XT is [d][n] float32 and finite. */
int bbbp_xgb_bin(void* stream, const float* XT, int n, int d, const float* cuts, int cut_stride, uint8_t* bins);
/* Fit every problem, all side by side: rounds of four launches, one tree level per round and problem, enqueued in blocks; between blocks
 * the word `alive_device` is read (the only host read), and the call returns when no problem grows any more: the stream is then idle.
 * `problems` is a host array, `problems_device` the same bytes in device memory.  A problem's numbers do not depend on what else is in
 * the batch: every sum is an integer sum or has a fixed order. */
int bbbp_xgb_fit(void* stream, const bbbp_xgb_problem* problems, const bbbp_xgb_problem* problems_device, int n_problems, int* alive_device);
/* For tools/bench_xgb.py, per host thread: with the profile on, bbbp_xgb_fit puts every split launch between two events; bbbp_xgb_fit_last
 * gives the last fit's sum of those times (0 with the profile off) and the number of launches it enqueued.  Returns the previous setting. */
int bbbp_xgb_fit_profile(int enable);
int bbbp_xgb_fit_last(double* split_ms, long* launches);

/* ---- xgbc fit: histogram-boosted classification trees, XGBoost's hist updater for binary:logistic (csrc/xgbc.hip) -------------------
 * XGBClassifier of the classification stack (Models/model_opt_20250130.py:445-456).  bbbp_amd/xgb.py states the algorithm and composes
 * XGBClassifier / fit_classifiers / randomized_search_cv from these.  Everything is bbbp_xgb_fit's -- the byte features (bbbp_xgb_bin makes
 * them), the node arrays, the ids, the limits BBBP_XGB_FIT_MAX_* -- but: y holds the targets 0.0 / 1.0; a row's gradient and hessian are
 * p - y and p (1 - p) in float32 with p = sigmoid32(margin), a float32 sigmoid made of IEEE float64 operations only; a node's hessian
 * sum is H = 2^-48 R with R the exact integer sum of max(1, llrint(h 2^48)), and sum_hessian records (float)H; a boundary is a candidate
 * iff either side holds a row, R >= 1 and H >= min_child_weight; a child is searched iff it has two rows.  With subsample_threshold != 0
 * tree t uses row i (its position in the problem) iff the high 32 bits of mix(mix(mix(seed + 0x9E3779B97F4A7C15) + t) + i) are below the
 * threshold (mix: the splitmix64 finaliser); the other rows have gradient and hessian 0 in that tree and still take their leaf's value; a
 * node without a used row is a leaf of weight -0.0.  With col_mask, tree t may split on feature f iff bit f % 32 of
 * col_mask[t * col_mask_stride + f / 32] is set. */
typedef struct bbbp_xgbc_problem {
    const uint8_t* bins;                       /* [d][n] */
    const float* cuts;                         /* [d][cut_stride] */
    const float* y;                            /* [n]: 0.0 / 1.0 */
    int n, d, cut_stride;
    int n_estimators, max_depth;
    uint32_t subsample_threshold;              /* floor(subsample 2^32); 0: every row is used */
    double reg_lambda, gamma, min_child_weight;
    float learning_rate, base_margin;          /* base_margin: the margin every row starts from */
    uint64_t seed;
    const uint32_t* col_mask;                  /* [n_estimators][col_mask_stride], or null: every feature is eligible */
    int col_mask_stride;                       /* >= ceil(d / 32) */
    void* work;                                /* bbbp_xgbc_fit_work_bytes(n, d) bytes, 16-byte aligned; need not be initialised */
    int* left; int* right; int* feature; float* cond; float* base_weight; float* loss_change; float* sum_hessian;      /* [n_estimators][capacity] */
    int* tree_nodes;                           /* [n_estimators]; -1 from the first tree on in which an index left its array (a defect) */
    float* margin;                             /* [n]: the training rows' margins after the last tree */
} bbbp_xgbc_problem;
/* Node slots per tree and bytes of a problem's `work`, as for bbbp_xgb_fit (0 with a message outside the limits). */
int bbbp_xgbc_fit_tree_capacity(int n, int max_depth);
size_t bbbp_xgbc_fit_work_bytes(int n, int d);
/* Fit every problem, all side by side, in bbbp_xgb_fit's rounds; a problem's numbers do not depend on what else is in the batch. */
int bbbp_xgbc_fit(void* stream, const bbbp_xgbc_problem* problems, const bbbp_xgbc_problem* problems_device, int n_problems, int* alive_device);
/* proba [m][2] float32: proba[i][1] = sigmoid32(margin[i]), proba[i][0] = 1 - proba[i][1] in float32. */
int bbbp_xgbc_proba(void* stream, const float* margin, long m, float* proba);

/* ---- cat fit: boosted oblivious (symmetric) regression trees, CatBoost's Plain boosting for RMSE (csrc/cat.hip) ----------------------
 * CatBoostRegressor of the logBB stack (Models/multi_input_data_regression_opt_transformer_cnn_20250108.py:192-195).  bbbp_amd/cat.py
 * states the algorithm and composes CatBoostRegressor / fit_regressors from these.  A problem is one model being fitted.  Its features are
 * bbbp_xgb_bin's bytes; candidate (f, c), c < n_cuts[f], sends a row right iff bins[f][i] > c.  Tree t owns split_feature / split_bin
 * [t * depth, t * depth + tree_depth[t]) (the feature counts the columns of `bins`) and leaf_values / leaf_weights
 * [t << depth, (t << depth) + (1 << tree_depth[t])); bit i of a leaf's index is the outcome of the tree's split i (CatBoost's order); an
 * empty leaf has value 0.0 and weight 0.  A tree is shallower than `depth` only when no unused (feature, cut) pair is left. */
#define BBBP_CAT_FIT_MAX_N 8192
#define BBBP_CAT_FIT_MAX_D 65536
#define BBBP_CAT_FIT_MAX_DEPTH 16
#define BBBP_CAT_FIT_MAX_TREES 10000
typedef struct bbbp_cat_problem {
    const uint8_t* bins;                       /* [d][n] */
    const int* n_cuts;                         /* [d]: the cuts of every feature, 1..255 */
    const double* y;                           /* [n] */
    int n, d;
    int iterations, depth;
    double l2_leaf_reg, learning_rate, bias;   /* bias: the mean of y, formed by the caller */
    void* work;                                /* bbbp_cat_fit_work_bytes(n, d, depth) bytes, 16-byte aligned; need not be initialised */
    int* split_feature; int* split_bin;        /* [iterations][depth] */
    double* leaf_values; int* leaf_weights;    /* [iterations][1 << depth] */
    int* tree_depth;                           /* [iterations]; -1 from the first tree on in which an index left its array (a defect) */
    double* approx;                            /* [n]: the training rows' approximations (leaf sums + bias) after the last tree */
} bbbp_cat_problem;
/* Bytes of a problem's `work` (0 with a message outside the limits above). */
size_t bbbp_cat_fit_work_bytes(int n, int d, int depth);
/* Fit every problem, all side by side: per tree and level three launches (split, choose, partition) and one more per tree (update), all
 * enqueued without a host read; the call returns when the stream is idle.  `problems` is a host array, `problems_device` the same bytes in
 * device memory.  A problem's numbers do not depend on what else is in the batch: every sum is an integer sum or has a fixed order. */
int bbbp_cat_fit(void* stream, const bbbp_cat_problem* problems, const bbbp_cat_problem* problems_device, int n_problems);
/* For tools/bench_cat.py, per host thread: with the profile on, bbbp_cat_fit puts every split launch between two events and waits for the
 * stream after every tree; bbbp_cat_fit_last gives the last fit's sum of those times (0 with the profile off) and the number of launches
 * it enqueued.  Returns the previous setting. */
int bbbp_cat_fit_profile(int enable);
int bbbp_cat_fit_last(double* split_ms, long* launches);

/* ---- catc fit: boosted oblivious (symmetric) classification trees, CatBoost's Plain boosting for Logloss (csrc/catc.hip) ---------------
 * CatBoostClassifier of the classification stack (Models/model_opt_20250130.py:413-457).  bbbp_amd/cat.py states the algorithm and
 * composes CatBoostClassifier / fit_classifiers / randomized_search_cv from these.  Everything is bbbp_cat_fit's -- the byte features, the
 * split and leaf arrays, the leaf order, the limits BBBP_CAT_FIT_MAX_* -- but: t holds the targets 0.0 / 1.0; a row's gradient and hessian
 * are t - p and p (1 - p) in float64 with p = sigmoid64(approx), a float64 sigmoid made of IEEE operations only; tree k gives row i (its
 * position in the problem) the weight weights[k * weight_stride + i] / 2^16 in the split scores, 1 <= weights < 2^22 (the caller draws
 * them: cat.py's Bayesian bootstrap); with weights null every weight is 2^16.  A part's gradient and weight sums are exact integer sums
 * (|gradient 2^k weight| < 2^50, at most 8 192 rows).  A leaf's value is one unweighted Newton step, learning_rate (G / (H + l2_leaf_reg)),
 * H = 2^-BBBP_CATC_HESS_BITS times the exact integer sum of max(1, llrint(h 2^BBBP_CATC_HESS_BITS)); leaf_weights records the row count. */
#define BBBP_CATC_HESS_BITS 48
typedef struct bbbp_catc_problem {
    const uint8_t* bins;                       /* [d][n] */
    const int* n_cuts;                         /* [d]: the cuts of every feature, 1..255 */
    const double* t;                           /* [n]: 0.0 / 1.0 */
    const uint32_t* weights;                   /* [iterations][weight_stride], or null: every row weighs 2^16 in every tree */
    long weight_stride;                        /* >= n */
    int n, d;
    int iterations, depth;
    double l2_leaf_reg, learning_rate, bias;   /* bias: every row's approximation before the first tree, formed by the caller */
    void* work;                                /* bbbp_catc_fit_work_bytes(n, d, depth) bytes, 16-byte aligned; need not be initialised */
    int* split_feature; int* split_bin;        /* [iterations][depth] */
    double* leaf_values; int* leaf_weights;    /* [iterations][1 << depth] */
    int* tree_depth;                           /* [iterations]; -1 from the first tree on in which an index left its array (a defect) */
    double* approx;                            /* [n]: the training rows' raw values (leaf sums + bias) after the last tree */
} bbbp_catc_problem;
/* Bytes of a problem's `work` (0 with a message outside the limits BBBP_CAT_FIT_MAX_*). */
size_t bbbp_catc_fit_work_bytes(int n, int d, int depth);
/* Fit every problem, all side by side, in bbbp_cat_fit's launches; a problem's numbers do not depend on what else is in the batch. */
int bbbp_catc_fit(void* stream, const bbbp_catc_problem* problems, const bbbp_catc_problem* problems_device, int n_problems);
/* For tools/bench_catc.py: as bbbp_cat_fit_profile / bbbp_cat_fit_last, for bbbp_catc_fit. */
int bbbp_catc_fit_profile(int enable);
int bbbp_catc_fit_last(double* split_ms, long* launches);
/* proba [m][2] float64: proba[i][1] = sigmoid64(raw[i]), proba[i][0] = 1 - proba[i][1] in float64; one launch. */
int bbbp_catc_proba(void* stream, const double* raw, long m, double* proba);

/* ---- rf fit: random-forest classification trees fitted by exact split search (csrc/rf.hip) --------------------------------------
 * RandomForestClassifier and DecisionTreeClassifier of the classification stack (Models/model_opt_maccs.py:124-200): two classes, Gini,
 * bootstrap rows as integer weights, max_features candidate features per node.  bbbp_amd/random_forest.py composes the classifiers and
 * grid_search_cv from these.  A descriptor is one tree; trees over one training matrix share XT and order0.  A tree owns capacity =
 * 2 n - 1 slots of the seven node arrays; nodes are numbered level by level from the root 0, children are tree-relative, -1 marks a
 * leaf (feature 0, threshold -2 there); value / value0 are the weighted class-1 / class-0 shares of every node, inner nodes included;
 * n_node_samples counts distinct rows.  Depth is limited by the rows alone.  All random choices come from bbbp_rf_hash: the tree's key
 * is hash(seed, tree_index), a child's key hash(key, side), bootstrap draw j is hash(hash(key(root), 0xB007), j) mapped to [0, n) by
 * multiply-high, a node's candidates are the max_features non-constant features with the lowest hash(key, 2 + f). */
#define BBBP_RF_FIT_MAX_N 8192
#define BBBP_RF_FIT_MAX_D 1024
#define BBBP_RF_MAX_WALK 8192            /* steps of one tree walk in the predict kernel; a longer walk yields NaN */
typedef struct bbbp_rf_tree {
    const float* XT;                           /* [d][n]: the training matrix, float32, one feature after the other */
    const int* order0;                         /* [d][n]: per feature the row indices sorted stably by value */
    const double* y;                           /* [n], 0.0 / 1.0 */
    int n, d;
    int max_depth;                             /* >= 1; any value >= n means unlimited */
    int min_samples_split, min_samples_leaf, max_features, bootstrap;
    int tree_index;                            /* the tree's number within its forest: a forest of fewer trees is a prefix */
    unsigned long long seed;
    void* work;                                /* bbbp_rf_fit_work_bytes(n, d, max_features) bytes, 16-byte aligned; need not be initialised */
    int* left; int* right; int* feature; int* n_node_samples; double* threshold; double* value; double* value0;      /* [capacity] */
    int* n_nodes;                              /* [1]: the tree's node count; -1 when an index left its array (a defect) */
} bbbp_rf_tree;
/* Node slots per tree, 2 n - 1 (0 with a message outside 2..BBBP_RF_FIT_MAX_N). */
int bbbp_rf_fit_tree_capacity(int n);
/* Bytes of a tree's `work` (0 with a message for n < 2, d < 1, n > BBBP_RF_FIT_MAX_N, d > BBBP_RF_FIT_MAX_D or max_features outside 1..d). */
size_t bbbp_rf_fit_work_bytes(int n, int d, int max_features);
/* The one hash behind every random choice of a fit: splitmix64's finaliser, mix(mix(a) + 0x9e3779b97f4a7c15 (b + 1)). */
unsigned long long bbbp_rf_hash(unsigned long long a, unsigned long long b);
/* Grow every tree, all side by side, one level per round of six launches.  Rounds are enqueued in blocks of eight; after each block the
 * word *alive_device (device memory, one int) is read back: the only host read before the result.  `trees` is a host array,
 * `trees_device` the same bytes in device memory.  A tree's numbers do not depend on what else is in the batch. */
int bbbp_rf_fit(void* stream, const bbbp_rf_tree* trees, const bbbp_rf_tree* trees_device, int n_trees, int* alive_device);
/* out[q] = (sum over the first n_trees trees, in tree order, of p0[leaf], of p1[leaf]) / n_trees for query rows X [m][d] float32
 * (scikit-learn's forest arithmetic).  Children are absolute indices into the node arrays, root[t] is tree t's first node; a row goes
 * left when (double)x[feature] <= threshold.  The walk stops at a node whose depth reaches max_depth or whose n_node_samples is below
 * min_samples_split (the pruned view of a tree grown without those limits) and after BBBP_RF_MAX_WALK steps. */
int bbbp_rf_predict_proba(void* stream, const float* X, long ld, int m, int d, const int* left, const int* right, const int* feature,
                          const double* threshold, const double* p0, const double* p1, const int* n_node_samples, const int* root,
                          int n_trees, int max_depth, int min_samples_split, double* out);
/* Regression trees under the squared-error criterion (RandomForestRegressor / DecisionTreeRegressor of the logBB stack,
 * Models/multi_input_data_regression_opt_transformer_cnn_opt.py:163-165): bbbp_rf_fit with the same descriptor, rounds, bootstrap, feature
 * draw, valid positions, thresholds and numbering.  y [n] holds integers q with |q| <= 2^49 as float64 (the caller rounds its targets to a
 * dyadic grid, q = rint(y 2^s), and scales the values back by 2^-s).  With S = sum w q (an exact int64) and W = sum w over a node's rows:
 * value = (double)S / (double)W, value0 = (double)W; a node whose targets are all one integer is a leaf; a position scores
 * (double)S_L (double)S_L / (double)W_L + (double)S_R (double)S_R / (double)W_R, every operation rounded to nearest, none fused.
 * `work` takes bbbp_rf_fit_regression_work_bytes(n, d, max_features) bytes: bbbp_rf_fit_work_bytes' plus 18 n for the rows' w q, w and the
 * nodes' S.  The limits BBBP_RF_FIT_MAX_N / _MAX_D and every argument check are bbbp_rf_fit's and run before any GPU call. */
size_t bbbp_rf_fit_regression_work_bytes(int n, int d, int max_features);
int bbbp_rf_fit_regression(void* stream, const bbbp_rf_tree* trees, const bbbp_rf_tree* trees_device, int n_trees, int* alive_device);
/* out[q] = (sum over the first n_trees trees, in tree order, of value[leaf]) / n_trees, float64 [m] (scikit-learn's regression forest):
 * bbbp_rf_predict_proba's walk and limits with one value per node. */
int bbbp_rf_predict_mean(void* stream, const float* X, long ld, int m, int d, const int* left, const int* right, const int* feature,
                         const double* threshold, const double* value, const int* n_node_samples, const int* root, int n_trees,
                         int max_depth, int min_samples_split, double* out);

/* ---- isolation forest: random trees on sub-samples, fitted and walked on the GPU (csrc/iforest.hip) ------------------------------
 * IsolationForest(contamination=0.05, random_state=42) of the regression stack's preprocessing
 * (Descriptors/multi_input_data_preprocess_maccs_opt_IsolationForest*.py, create_descriptors_PCA_regression_{1,2,3}.py): the step behind
 * PCA.  bbbp_amd/isolation_forest.py composes the estimator from these.  The rule is scikit-learn's ExtraTreeRegressor(max_features=1,
 * splitter="random") as IsolationForest uses it, every random choice one bbbp_rf_hash:
 *   key(root of tree t) = hash(hash(seed, 0x1F0BE57), t); key(child) = hash(key, side), side 0 left and 1 right;
 *   the tree's rows: the max_samples rows i of [0, n) with the lowest hash(hash(key(root), 0x5A3B1E), i), kept in ascending order
 *     (the hash is a bijection of i: no two rows tie);
 *   a node is a leaf with fewer than 2 rows, at depth max_depth = ceil(log2(max(max_samples, 2))), or when every feature is constant on
 *     its rows (float32 max <= min + 1e-7f, scikit-learn's FEATURE_THRESHOLD); there is no rule on a target's impurity;
 *   otherwise its feature is the first in ascending order of hash(key, 2 + f) that is not constant on its rows, and its threshold is
 *     thr = lo + (hi - lo) * u in float64, lo / hi the feature's float32 minimum / maximum over the rows, u = (hash(key, 0x7412E5) >> 11)
 *     * 2^-53, the subtraction, the product and the sum each rounded once and none fused; thr >= hi gives thr = lo;
 *   a row goes left when (double)x <= thr; nodes are numbered level by level from the root 0, the children of a level's split nodes in
 *     their parents' order, left before right; children are tree-relative, -1 marks a leaf (feature 0, threshold -2 there);
 *     n_node_samples counts rows.
 * A tree owns capacity = 2 max_samples - 1 slots of the five node arrays and max_samples entries of `samples`. */
#define BBBP_IFOREST_MAX_SAMPLES 1024    /* rows of one tree: four row slots per thread of the 256-thread work-group */
#define BBBP_IFOREST_MAX_D 1024
#define BBBP_IFOREST_MAX_N 2147483392    /* rows of X: int row indices, whole passes of 256 */
/* Node slots per tree, 2 max_samples - 1 (0 with a message outside 1..BBBP_IFOREST_MAX_SAMPLES). */
int bbbp_iforest_tree_capacity(int max_samples);
/* The fit's work area is its work-group's LDS (row permutation, node segments and node tables of two levels): the caller allocates
 * nothing but the outputs.  Returns the LDS bytes one work-group takes, 92 max_samples rounded up per array to 16 (0 with a message
 * outside 1..BBBP_IFOREST_MAX_SAMPLES). */
size_t bbbp_iforest_work_bytes(int max_samples);
/* Grow trees 0 .. n_trees - 1 of the forest of `seed` over X [n][d] float32 (row stride ld), all in one launch,
 * one work-group per tree, without a host read.  left, right, feature, n_node_samples [n_trees][capacity], threshold
 * [n_trees][capacity], samples [n_trees][max_samples] (the tree's rows, ascending), n_nodes [n_trees]: the tree's node count, -1 when
 * an index left its array (a defect).  1 <= max_samples <= min(n, BBBP_IFOREST_MAX_SAMPLES), n <= BBBP_IFOREST_MAX_N, d <= BBBP_IFOREST_MAX_D, n_trees <= 65535;
 * every argument is checked before any GPU call.  A tree's numbers do not depend on what else is in the launch. */
int bbbp_iforest_fit(void* stream, const float* X, long ld, int n, int d, int max_samples, int n_trees, unsigned long long seed,
                     int* left, int* right, int* feature, int* n_node_samples, double* threshold, int* samples,
                     int* n_nodes);
/* out[q] = sum over the trees, in tree order and in float64, of term[leaf] for query rows X [m][d] float32: bbbp_rf_predict_mean's walk
 * ((double)x[feature] <= threshold goes left, absolute child indices, root[t] tree t's first node, at most BBBP_RF_MAX_WALK steps, a
 * longer walk yields NaN) without limits and without the division. */
int bbbp_iforest_path_sum(void* stream, const float* X, long ld, int m, int d, const int* left, const int* right, const int* feature,
                          const double* threshold, const double* term, const int* root, int n_trees, double* out);

/* ---- Bernoulli naive Bayes on bits: batched counting and joint log-likelihoods (csrc/bnb.hip) -----------------------------------------
 * BernoulliNB() of the classification stack (Models/model_maccs.py:257-267: alpha x binarize under five folds, then a learning curve).
 * bbbp_amd/naive_bayes.py composes the estimator, fit_masks, grid_search_cv and learning_curve from these; the log tables are formed
 * on the host from the integer counts, so alpha is no argument here.  Words are 64 bits, bit b of word w stands for index 64 w + b, and
 * the bits past the last index of a word vector are 0. */
#define BBBP_BNB_MAX_D 1048576           /* features: the pack grid's second dimension is ceil(d / 64) */
#define BBBP_BNB_MAX_THRESHOLDS 1024
#define BBBP_BNB_MAX_PROBLEMS 65535      /* masks, pairs or jll problems of one launch */
#define BBBP_BNB_MAX_ITEMS 2147483647L   /* counts of one launch: 2 d n_pairs + 2 n_masks */
/* bit = X[i][j] > thresholds[t] (strict, sklearn.preprocessing.binarize) for X [n][d] float32 or float64 (x_dtype: BBBP_DTYPE_*, unit
 * inner stride, row stride ld).  For float32 X the threshold is rounded to float32 first, numpy's rule for an array compared with a
 * Python float.  Two layouts, either may be NULL: planes [T][d][ceil(n/64)] (feature-major: a word holds 64 rows of one feature) and
 * rowwords [T][n][ceil(d/64)] (row-major: a word holds 64 features of one row).  Every word of both is written whole, padding bits as 0:
 * nothing has to be cleared beforehand.  *flag (device, 0 on entry) is set to 1 when X holds NaN or infinity; such an entry packs as 0.
 * thresholds is a device array.  n <= 2^31 - 1, d <= BBBP_BNB_MAX_D, T <= BBBP_BNB_MAX_THRESHOLDS. */
int bbbp_bnb_pack(void* stream, const void* X, int x_dtype, long ld, int n, int d, const double* thresholds, int n_thresholds,
                  unsigned long long* planes, unsigned long long* rowwords, int* flag);
/* Every count of a batch in one launch.  masks [M][2][ceil(n/64)]: a row subset intersected with class 0 and with class 1.  Pair q is
 * (pair_mask[q], pair_threshold[q]), device arrays of n_pairs ints.
 *   feature_count[q][c][j] = sum_w popcount(planes[t][j][w] & masks[m][c][w])   int32 [n_pairs][2][d]
 *   class_count[m][c]      = sum_w popcount(masks[m][c][w])                      int32 [M][2]
 * Exact integers, one wave per count; a pair that names a mask or a threshold outside the batch yields -1 and reads nothing.
 * M, n_pairs <= BBBP_BNB_MAX_PROBLEMS and 2 d n_pairs + 2 M <= BBBP_BNB_MAX_ITEMS. */
int bbbp_bnb_count(void* stream, const unsigned long long* planes, int n, int d, int n_thresholds, const unsigned long long* masks,
                   int n_masks, const int* pair_mask, const int* pair_threshold, int n_pairs, int* feature_count, int* class_count);
/* Joint log-likelihoods of a batch in one launch, one lane per (problem, query row).  Problem p has the table w[p][2][d], the constant
 * c[p][2] and four longs problems[p] = {threshold index, row_begin, n_rows, out_begin}: its query rows are rows[row_begin .. + n_rows)
 * (indices into [0, n)), or with row_begin < 0 the rows 0 .. n_rows - 1, and its results are out[out_begin .. + n_rows)[2].
 *   out[.][k] = ((0.0 + w[p][k][j1]) + w[p][k][j2] + ...) + c[p][k],  j1 < j2 < ... the set bits of the row in rowwords[t]
 * float64 additions, each rounded once, in exactly this order.  rows has n_row_entries ints (may be NULL with 0), out has n_out pairs of
 * doubles, max_rows is the largest n_rows.  A problem whose threshold index or rows leave their arrays yields NaN.
 * n_problems <= BBBP_BNB_MAX_PROBLEMS. */
int bbbp_bnb_jll(void* stream, const unsigned long long* rowwords, int n, int d, int n_thresholds, const double* w, const double* c,
                 const long* problems, int n_problems, const int* rows, long n_row_entries, int max_rows, long n_out, double* out);

/* ---- resampling of imbalanced classes: SMOTE's synthesis and Tomek links (csrc/smote.hip) ------------------------------------------------
 * SMOTE(random_state=42) / SMOTETomek(random_state=42) of the classification stack (Models/model_opt_maccs.py, model_opt_20250130.py): the
 * step between PCA and the learners.  bbbp_amd/imbalance.py composes the estimators from these, bbbp_knn_f64 and the host's
 * numpy.random.RandomState draws. */
/* out[j][:] = Xc[r][:] + steps[j] * (Xc[b][:] - Xc[r][:]) for j < n_new, r = idx[j] / k, b = nn[r][idx[j] % k].  Xc [n_c][d] float32 or
 * float64 (x_dtype: BBBP_DTYPE_*, unit inner stride, row stride ldx, any base alignment), nn [n_c][k] dense, idx [n_new] in [0, n_c k),
 * steps [n_new] float64, out [n_new][d] of Xc's type with row stride ldo.  Rounding is numpy's for `X[rows] + steps[:, None] * diffs`:
 * float64 rows: difference, product and sum each rounded once in float64; float32 rows: the difference rounded to float32, product and
 * sum in float64 on the widened values, the sum rounded once to float32.  Nothing is fused.  An idx or nn entry outside its array yields a
 * row of NaN and reads nothing.  n_new = 0 or d = 0 is a no-op; otherwise n_c > k. */
int bbbp_smote_synth(void* stream, const void* Xc, int x_dtype, long ldx, int n_c, const long* nn, const long* idx, const double* steps,
                     int k, int n_new, int d, void* out, long ldo);
/* keep[i] = 0 when row i is a member of a Tomek link (y[nn1[i]] != y[i] and nn1[nn1[i]] == i) and remove[y[i]] != 0, else 1, for i < n.
 * nn1 [n]: the nearest other row of every row; y [n]: labels in [0, n_classes); remove [n_classes] bytes.  Every byte of keep is
 * written.  An index or a label outside its array is no link. */
int bbbp_tomek_links(void* stream, const long* nn1, const int* y, const unsigned char* remove, int n_classes, int n, unsigned char* keep);

/* ---- preprocessing: StandardScaler and PolynomialFeatures in float64 (csrc/scaler.hip, csrc/poly.hip) -------------------------------------
 * The first step of every pipeline of the reference (Models/model_opt_maccs.py:104: StandardScaler -> PCA -> SMOTE -> learners) and the
 * expansion of the regression feature scripts (Descriptors/multi_input_data_preprocess_maccs_opt_IsolationForest_fixed_1.py:105-134).
 * bbbp_amd/preprocessing.py composes the estimators from these.  Common to the three entry points: X [n][d] float64 with unit inner
 * stride and row stride ldx >= d, read in place at any 8-byte aligned base; flag: one int that the call sets to 0 and a kernel ORs to 1
 * when it meets a NaN or an infinity in X (bbbp_scaler_apply and bbbp_poly_expand accept NULL: no check). */
/* Column moments of one batch, merged with the moments of the rows seen before: scikit-learn 1.7's _incremental_mean_and_var and
 * _is_constant_feature, every operation rounded once and in this order.  Per column, rows in order: S = sum x from 0.0; T = S / n;
 * corr = sum (x - T), sq = sum (x - T) * (x - T); u_new = sq - (corr * corr) / n.  last_n == 0 (last_mean, last_var may be NULL):
 * mean = (0.0 + S) / n, u = u_new, N = n.  Otherwise last_sum = last_mean * last_n, N = last_n + n, mean = (last_sum + S) / N, r = last_n / n,
 * u = (last_var * last_n + u_new) + (r / N) * (y * y) with y = last_sum / r - S (last_var NULL: taken as 0, for a caller that keeps no
 * variance).  var = u / N; scale = 1.0 where var <= (N * eps) * var + ((N * mean) * eps)^2, eps = 2^-52, else sqrt(var).  mean, var and
 * scale [d] are written in full.  One launch, no host read.  n >= 1, d >= 1. */
int bbbp_scaler_moments(void* stream, const double* X, long ldx, int n, int d, const double* last_mean, const double* last_var, long last_n,
                        double* mean, double* var, double* scale, int* flag);
/* out[i][j] = (X[i][j] - mean[j]) / scale[j] (inverse == 0) or X[i][j] * scale[j] + mean[j] (inverse == 1), two roundings; a NULL mean or
 * scale skips its step.  out [n][d] with row stride ldo >= d, 8-byte aligned; every element is written and nothing else.  Where both
 * bases are 16-byte aligned and both row strides even the accesses are 16 bytes wide.  n = 0 or d = 0 is a no-op. */
int bbbp_scaler_apply(void* stream, const double* X, long ldx, int n, int d, const double* mean, const double* scale, int inverse,
                      double* out, long ldo, int* flag);
/* out[i][p] for p < P from table [P][3] (int, dense): the row (f0, f1, f2) with -1 for an absent factor gives 1.0 when f0 == -1, else
 * X[i][f0], times X[i][f1] when f1 >= 0, times X[i][f2] when f2 >= 0: float64 products in that order, each rounded once.  out [n][P]
 * with row stride ldo >= P, 8-byte aligned; every element is written and nothing else.  The flag watches the one-factor columns.  A
 * factor outside [-1, d) reads nothing and yields NaN.  n = 0 is a no-op; d >= 1, P >= 1. */
int bbbp_poly_expand(void* stream, const double* X, long ldx, int n, int d, const int* table, int P, double* out, long ldo, int* flag);

/* ---- batched classification and regression scores (csrc/metrics.hip) ----------------------------------------------------------------------
 * evaluate_model of the classification scripts (Models/model_maccs.py, model_opt*.py: eight scores per fitted model) and the
 * mean_squared_error / r2_score pair of the regression scripts.  The device computes integers (confusion counts, Mann-Whitney pair counts)
 * and float64 sums in a fixed order; bbbp_amd/metrics.py forms the scores from them on the host.  Common to the three entry points:
 * M columns [M][n] with row stride ld (unit inner stride, any base alignment), one y vector [n], and seg [n] (may be NULL: every row in
 * segment 0): a segment id in [0, G) per row, any other value leaves the row out.  Results are per (column, segment).  Every output word is
 * written, so nothing has to be cleared; *flag (device, 0 on entry) is set to 1 when a float that takes part (a row of some segment) is NaN
 * or infinite.  Row tiles of BBBP_METRICS_TILE_ROWS rows go to work-groups of their own: with more than one tile, `work` receives one slab
 * of partial results per tile (bbbp_metrics_work_bytes; integer sums, so the result does not depend on any order) and a second launch adds
 * them; with one tile `work` may be NULL and there is one launch. */
#define BBBP_METRICS_DTYPE_U8 2          /* beside BBBP_DTYPE_F32 / _F64: hard predictions as 0 / 1 bytes (any non-zero byte is 1) */
#define BBBP_METRICS_MAX_COLUMNS 65535
#define BBBP_METRICS_MAX_GROUPS 64
#define BBBP_METRICS_TILE_ROWS 16384     /* confusion counts: rows per work-group */
#define BBBP_METRICS_PAIR_ROWS 256       /* pair counts: rows per work-group (one per lane) */
/* Bytes of `work` for n rows: what = 0 confusion counts, 1 pair counts.  0 when one tile suffices (confusion counts only). */
size_t bbbp_metrics_work_bytes(int what, int n_columns, int n, int n_groups);
/* counts[m][g] = (tn, fp, fn, tp) as int64 over the rows of segment g, with the prediction of row i of column m being
 * pred[m * ld + i] != 0 for bytes, and pred[m * ld + i] > thr[m] (strict; thr is a device array of M doubles, compared in float64) for
 * float32 / float64 scores.  y01 [n] bytes: the truth, non-zero is positive.  thr is not read for bytes and may be NULL. */
int bbbp_metrics_confusion(void* stream, const void* pred, int dtype, long ld, int n_columns, int n, const double* thr,
                           const unsigned char* y01, const int* seg, int n_groups, long long* counts, void* work, int* flag);
/* out[m][g] = (U2, P, N, nonfinite) as int64: P, N the positive and negative rows of segment g, nonfinite its rows whose score is NaN or
 * infinite, and U2 = sum over positive rows i of #{negative rows j of the segment: s_j < s_i} + #{...: s_j <= s_i}, so that
 * AUC = U2 / (2 P N).  Scores (dtype: float32, float64 or bytes) are compared as float64 values (-0.0 == 0.0; a NaN compares false).
 * Every pair is visited: no sort, no row limit, n^2 / 256 LDS tile passes per column.  work (bbbp_metrics_work_bytes(1, ...)) is needed. */
int bbbp_metrics_auc_pairs(void* stream, const void* score, int dtype, long ld, int n_columns, int n, const unsigned char* y01,
                           const int* seg, int n_groups, long long* out, void* work);
/* sse[m][g] = sum (y_i - p_i)^2 over the rows of segment g for column m (p float32 or float64, widened exactly), and once per segment
 * ystat[g] = (sum y_i, sum (y_i - ybar)^2 with ybar = (sum y_i) / count, count) as doubles.  One work-group of 256 lanes per (column,
 * segment): lane t adds its rows t, t + 256, ... in ascending order, then `v += shfl_down(v, off)` for off = 32 .. 1, then the four waves
 * in ascending order; every product, difference and sum is rounded once (no fused multiply-add). */
int bbbp_metrics_sq_sums(void* stream, const void* pred, int dtype, long ld, int n_columns, int n, const double* y, const int* seg,
                         int n_groups, double* sse, double* ystat, int* flag);

/* ---- the classifier stack's device glue (csrc/ensemble.hip) ---------------------------------------------------------------------------------
 * StackingClassifier(estimators, final_estimator=GradientBoostingClassifier(...), cv=5) and VotingClassifier(estimators, voting='soft') of the
 * classification scripts (Models/model_opt.py:208-222).  bbbp_amd/ensemble.py composes the two estimators from the base learners' fits and
 * these three entries, each one launch however many estimators and folds there are, each pinned bit for bit to tests/ensemble_numpy.py.
 * Every table exists twice: the host's copy, which the entry validates before the launch, and the same bytes on the device, which the kernel
 * reads; the caller keeps both, and what they point to, alive until the kernel is done.  Sources have unit inner stride inside a row, any
 * row stride (in elements) and any base alignment of their element type. */
#define BBBP_ENS_MAX_ENTRIES 65535       /* (estimator, fold) entries of one scatter */
#define BBBP_ENS_MAX_ESTIMATORS 65535    /* columns of one vote */
typedef struct bbbp_ens_source {
    const double* src;   /* device: element (i, col) at src[i * stride + col] */
    long stride, col;    /* stride >= col + 1 */
    const long* rows;    /* device: the destination row of every source row, count ids; NULL: row i goes to row i */
    long count;          /* source rows */
    long dst;            /* destination column in [0, n_columns) */
} bbbp_ens_source;
typedef struct bbbp_ens_column {
    const void* src;     /* device: doubles (soft vote: the pair at columns col, col + 1) or bytes (hard vote: the 0 / 1 prediction at col) */
    long stride, col;    /* stride >= col + 2 (soft vote), col + 1 (hard vote) */
} bbbp_ens_column;
/* meta[rows[i]][dst] = src[i * stride + col] for every entry and i < count; meta [n][n_columns] float64 with row stride ld.  Nothing is
 * cleared and nothing is added: the entries of one destination column must write every one of its n rows exactly once (a fold's test rows
 * partition the rows), which is checked here on rows_host, the host's copy of the row ids of all entries that have some, concatenated in
 * entry order (NULL when no entry has row ids); a row id outside [0, n), a cell written twice or never is BBBP_ERR_ARG.  The kernel has no
 * bounds check of its own.  n = 0 is a no-op. */
int bbbp_ens_meta_scatter(void* stream, const bbbp_ens_source* table, const void* table_dev, int n_entries, const long* rows_host, int n,
                          int n_columns, double* meta, long ld);
/* np.average of n_estimators probability pairs per row over the estimator axis: s = P_0 (* w_0), s = s + P_j (* w_j) in estimator order,
 * out[i] = s / scl; without weights (NULL; device array of n_estimators doubles otherwise) out[i] = s / n_estimators and scl is not read.
 * scl is the sum of the weights as the caller's numpy forms it (pairwise from eight on).  Every product, sum and quotient is rounded once,
 * nothing is fused.  out [m][2] float64 dense; label [m] bytes: 1 when the second average is the first maximum (numpy's argmax, a NaN
 * counting as a maximum), else 0.  m = 0 is a no-op. */
int bbbp_ens_soft_vote(void* stream, const bbbp_ens_column* cols, const void* cols_dev, int n_estimators, const double* weights, double scl,
                       int m, double* out, unsigned char* label);
/* np.bincount(predictions, weights=) per row: counts[i][k] = sum over j in estimator order of w_j (1.0 without weights) where the byte of
 * estimator j is k (any non-zero byte is 1), added in float64 from 0.0; label as for the soft vote: ties go to class 0.  m = 0 is a no-op. */
int bbbp_ens_hard_vote(void* stream, const bbbp_ens_column* cols, const void* cols_dev, int n_estimators, const double* weights, int m,
                       double* counts, unsigned char* label);

/* ---- optional per-section timing (HIP events on the launch stream; used by bench.py's roofline leg) ----
 * enable(1), run steps, synchronise the stream, collect(ms_sum[n], count[n]) with n = num_sections(). */
int bbbp_set_partition(int reserved_cus, size_t small_lds_pad);   /* CU partition knob, see csrc/common.h */
/* CUs kept out of every persistent grid (conv / GEMM grids are sized from the CU count): room for the collective library's kernels
 * beside the persistent work-groups in a multi-GPU run.  Initial value BBBP_COMM_CUS (default 0); ignored when fewer than 64 CUs would
 * remain.  bench.py's N-rank diagnostic pass measures 0 against 8 and keeps the faster one.  Returns the previous value. */
int bbbp_set_comm_cus(int n);
/* The head / fusion-block input-gradient chain of bbbp_mixed_backward as two fused launches instead of ten (default on since
 * round 2: 3.32 -> 3.27 ms per step at B = 512).  Returns the previous setting.  Initial value: BBBP_FUSED_HEAD_BWD. */
int bbbp_set_fused_head_bwd(int on);
/* Alternative schedules of the fingerprint encoder, a bit mask (default 0: every one measured slower than the launch-per-op chain, see
 * DESIGN.md section 3; initial value BBBP_FUSED_ENCODER).  All of them fill the same workspace and draw the same dropout masks.
 * bit 0: the row-local stretches of a layer (out_proj .. LayerNorm2 + the next in_proj forward; LayerNorm2 backward .. out_proj input
 *        gradient backward) as ONE launch each (csrc/encoder.hip: enc_row_*_kernel) instead of 6 + 6, for d_model <= 192;
 * bit 1: batches of at most 128 molecules, one head, d_model <= 176: the whole FORWARD chain of the encoder (all layers + fingerprint_fc)
 *        as one persistent launch (enc_sliced_fwd_kernel: 16-row blocks shared by column-slicing work-groups, barriers through counters
 *        in the workspace);
 * bit 2: the same for the BACKWARD input-gradient chain (enc_sliced_bwd_kernel); the weight gradients stay leaf launches.
 * Returns the previous mask. */
int bbbp_set_fused_encoder(int mode);
/* One-head encoder layers (nhead 1: a prime fingerprint width such as 167) on the launch-per-op schedule: out_proj folded into the value
 * projection (csrc/fold.hip).  out_proj(Pd V) = Pd (x (Wo Wv)^T + 1 (Wo bv)^T) + bo, so in_proj produces [Q | K | VW] with the folded
 * weight block W' = Wo Wv (one launch per step for all layers), the out_proj GEMM leaves the forward chain, its input-gradient GEMM leaves
 * the backward chain, and its weight gradient is unfolded from the in_proj weight gradient's V block (dWo = dW' Wv^T + db' bv^T,
 * d[Wv | bv] = Wo^T [dW' | db'], dbo = column sums).  The same function as nn.TransformerEncoderLayer (...20250113.py:75-78) up to
 * float32 rounding of the reassociated products.  A bit mask, default 3 (initial value BBBP_FOLD_OUTPROJ): bit 0 the launch-per-op
 * schedule with materialised probabilities (training steps, eval batches below 2048 rows); bit 1 also the forward-only split-bf16
 * attention kernel of 2048+ row plans (no dropout there: bo rides in b'; those plans run on one stream); 0 keeps
 * the reference's operation order.  Never applied with the small-head fused attention, the exact-global-batch mode or
 * bbbp_set_fused_encoder != 0.  Changes the workspace layout: set it before bbbp_mixed_workspace_bytes / the forward call of a step.
 * Returns the previous mask. */
int bbbp_set_fold_outproj(int mask);
/* Fused flash-style self-attention (csrc/attention.hip, csrc/attention_b3.hip), a bit mask (default 13, initial value BBBP_FLASH_ATTENTION):
 * bit 0: many heads of head_dim 8 / 16 (F = 2048: 256 x 8), one work-group per head, scores in registers, no [nhead, B, B] tensors;
 * bit 1: one wide head of 161 .. 176 columns (F = 167, nhead = 1), operands straight from global memory, everywhere -- correct but
 *        measured slower than the batched-GEMM + softmax schedule in the B = 512 .. 2048 training steps, hence opt-in;
 * bit 2: that kernel only where it is faster: forward-only (inference) plans of 2048 rows and more (screening batches);
 * bit 3: forward-only plans of 2048 rows and more (bit 4: from 256 rows, for tests) with a wide head (96 < head_dim <= 192) on the bf16 matrix pipe with split operands
 *        (attention_b3.hip: K / V^T tiles staged once per 128 queries, scores fed back as the second product's operand, key axis split
 *        over work-groups + a merge pass); takes precedence over bit 2.
 * 0 selects the batched GEMM + softmax schedule everywhere.  Returns the previous mask.  Changes the workspace layout: set it
 * before the forward call, not between forward and backward. */
int bbbp_set_flash_attention(int on);
/* The attention kernels behind that mask as ops of their own (csrc/attention.hip, csrc/attention_b3.hip; F.scaled_dot_product_attention of
 * nn.MultiheadAttention, R:75-78, sequence = the batch).  qkv [B][3F] = Q | K | V with head h at columns h * head_dim .. of each third, F = nhead *
 * head_dim; ctx [B][F]; lse [nhead][B] = logsumexp of the scaled scores; dropout element (h B + q) B + k of stream `seed` (bbbp_set_seed_base
 * applies).  bbbp_attention_supported: bit 0 the small-head kernels (nhead > 1, head_dim 8 or 16, B <= 960 / 512), bit 1 the wide-head
 * kernels (nhead <= 8, head_dim 161 .. 176), bit 2 the forward-only split-bf16 kernel (nhead <= 16, head_dim 97 .. 192); bbbp_attention_fwd / _bwd
 * run bit 0 where it is set, else bit 1, and return BBBP_ERR_ARG for any other shape.  `keep` (nullable, bbbp_attention_keep_bytes; 0 for
 * shapes of the wide-head kernels, which do not use it): [nhead][ceil(B/16)][ceil(B/16)][64] bytes, bit r of byte (q, kq) = the decision for
 * key 16 kt + 4 kq + r of query 16 qb + q; written by the forward pass when dropout_p > 0, read by the backward pass instead of drawing the
 * stream again (NULL there: redrawn, same decisions).  bbbp_attention_b3_fwd: no dropout, no lse; `workspace` of
 * bbbp_attention_b3_workspace_bytes (0: the key axis is not split, no merge pass). */
int bbbp_attention_supported(int B, int nhead, int head_dim);
size_t bbbp_attention_keep_bytes(int B, int nhead, int head_dim);
int bbbp_attention_fwd(void* stream, const float* qkv, float* ctx, float* lse, int B, int F, int nhead, float scale, float dropout_p,
                       uint64_t seed, uint8_t* keep);
int bbbp_attention_bwd(void* stream, const float* qkv, const float* ctx, const float* lse, const float* dctx, float* dqkv, int B, int F,
                       int nhead, float scale, float dropout_p, uint64_t seed, const uint8_t* keep);
size_t bbbp_attention_b3_workspace_bytes(int B, int nhead, int head_dim);
int bbbp_attention_b3_fwd(void* stream, const float* qkv, float* ctx, int B, int F, int nhead, float scale, float* workspace,
                          size_t workspace_bytes);
/* ---- the encoder layer outside attention, as ops of their own (csrc/fold.hip, csrc/encoder.hip; nn.TransformerEncoderLayer, R:75-78) ----
 * Thin entry points over the launchers bbbp_mixed_forward / _backward use: same kernels, same bits.  Every one refuses a null required
 * pointer, an unsupported width and an empty extent with BBBP_ERR_ARG before any HIP call.  The pointer lists are HOST arrays of device
 * pointers.
 * bbbp_outproj_fold_fwd, per layer l < layers (one head, F = 1 .. 255, at most 32 layers: bbbp_outproj_fold_supported): from in_proj
 * win[l] [3F][F] = Wq; Wk; Wv, bin[l] [3F], out_proj wo[l] [F][F] and bo[l] [F] (the list or an entry may be NULL: not added) the folded
 * wf[l] [3F][F] = Wq; Wk; Wo Wv, bf[l] [3F] = bq; bk; Wo bv (+ bo) and wvt[l] [F + 1][F] = [Wv | bv]^T.
 * bbbp_outproj_fold_bwd: the gradients unfolded from tdw [F][F] = dW', tdb [F] = db' and dz [B][F] (row stride lddz >= F), the gradient of
 * out_proj's output: g_outw [F][F] = dW' Wv^T + db' bv^T, g_outb [F] = column sums of dz, g_inw_v [F][F] | g_inb_v [F] = Wo^T [dW' | db'].
 * bbbp_ln_param_grad: dgamma[i] [cols] = sum_rows dy[i] * (z[i] - mean[i]) * rstd[i] and dbeta[i] [cols] = sum_rows dy[i] of n >= 1
 * LayerNorms over [rows][cols] tensors (twelve norms per launch). */
int bbbp_outproj_fold_supported(int F, int nhead, int layers);
int bbbp_outproj_fold_fwd(void* stream, int layers, int F, const float* const* win, const float* const* bin, const float* const* wo,
                          const float* const* bo, float* const* wf, float* const* bf, float* const* wvt);
int bbbp_outproj_fold_bwd(void* stream, int F, int B, const float* tdw, const float* tdb, const float* wo, const float* wvt, const float* dz,
                          int lddz, float* g_outw, float* g_outb, float* g_inw_v, float* g_inb_v);
int bbbp_ln_param_grad(void* stream, int n, const float* const* dy, const float* const* z, const float* const* mean,
                       const float* const* rstd, float* const* dgamma, float* const* dbeta, int rows, int cols);
/* The row-local stretch of a post-norm encoder layer as one launch per direction (bit 0 of bbbp_set_fused_encoder), for F = 4 .. 192 and
 * DFF >= 16 (bbbp_encoder_rows_supported).  Forward, per row of ctx / xin [B][F]:
 *   z1 = dropout1(ctx Wo^T + bo) + xin, y1 = LayerNorm(z1; g1, be1), hff = dropout2(relu(y1 W1^T + b1)) [B][DFF],
 *   z2 = dropout3(hff W2^T + b2) + y1, y2 = LayerNorm(z2; g2, be2), and when wn is not NULL outn[b][0 .. nn) = act(y2 Wn^T + bn) with row
 *   stride ldn >= nn (actn: 0 none, 1 ReLU); wn [nn][F].  Dropout site i scales element row * F + col (site 2: row * DFF + col) by the
 *   keep-scale of Philox stream seed_i, as bbbp_dropout does for a contiguous tensor (bbbp_set_seed_base applies); eps = 1e-5.
 * Backward, from dyout [B][F], the gradient of y2 -- read, or, when dqkv_up is not NULL (then win_up [3F][F] and dz1_up [B][F] too),
 * first written as dqkv_up [B][3F] win_up + dz1_up -- and the forward's z1, z2, hff, mean*, rstd*:
 *   dz2 (gradient of z2), dff = dropout3 of it, dhff = (dff W2) where hff > 0, times 1 / (1 - p), dy1 = dhff W1 + dz2, dz1 (gradient of
 *   z1), dsa = dropout1 of it, dctx = dsa Wo.  All [B][F] but dhff [B][DFF]. */
typedef struct bbbp_encoder_rows_fwd_desc {
    int B, F, DFF;
    float dropout_p;
    unsigned long long seed1, seed2, seed3;
    const float *ctx, *xin;
    const float *wo, *bo, *g1, *be1, *w1, *b1, *w2, *b2, *g2, *be2;
    const float *wn, *bn; float* outn; int nn, ldn, actn;          /* the next projection: optional */
    float *z1, *y1, *hff, *z2, *y2, *mean1, *rstd1, *mean2, *rstd2;
} bbbp_encoder_rows_fwd_desc;
typedef struct bbbp_encoder_rows_bwd_desc {
    int B, F, DFF;
    float dropout_p;
    unsigned long long seed1, seed3;
    const float *dqkv_up, *win_up, *dz1_up;                        /* stage 0: all three or none */
    float* dyout;
    const float *z2, *mean2, *rstd2, *g2, *w2, *hff, *w1, *z1, *mean1, *rstd1, *g1, *wo;
    float *dz2, *dff, *dhff, *dy1, *dz1, *dsa, *dctx;
} bbbp_encoder_rows_bwd_desc;
int bbbp_encoder_rows_supported(int F, int nhead, int dff);
int bbbp_encoder_rows_fwd(void* stream, const bbbp_encoder_rows_fwd_desc* d);
int bbbp_encoder_rows_bwd(void* stream, const bbbp_encoder_rows_bwd_desc* d);
/* Products that take the 128 x 128 tile plan (the F = 2048 encoder's GEMMs, the 65536-wide image FC): 1 (default; initial value
 * BBBP_GEMM_SPLIT_BF16) runs them on the bf16 matrix pipe with every float32 operand split into three bf16 pieces (six MFMAs per
 * k-step, f32 accumulate, float32 accuracy; csrc/gemm.hip: gemm_b3_kernel), 0 on the f32 MFMA.  Returns the previous setting. */
int bbbp_set_gemm_split_bf16(int on);
/* Split-K launches of the split-bf16 GEMM: 1 lets the K range that arrives last at an output tile sum the tile's slabs in split order
 * and apply the epilogue inside the GEMM launch (per-tile arrival counters, slabs written through to the coherence point), 0 (default;
 * initial value BBBP_GEMM_FOLD_REDUCE) runs the separate reduce kernel.  Both produce the same bits; the in-kernel form is measured
 * slower on MI355X.  Returns the previous setting. */
int bbbp_set_gemm_fold_reduce(int on);
/* Debug: shader cycles of work-group 0 / wave 0 of the last split-bf16 GEMM launched with BBBP_GEMM_B3_PROBE=1 in the environment:
 * [0] global-load issue, [1] LDS reads + MFMA block, [2] barrier after it, [3] split + LDS writes, [4] barrier after them, [5] all shader
 * cycles of that wave's K loop and [6] the same span in 100 MHz wall ticks (their ratio is the sustained shader clock). */
int bbbp_gemm_split_bf16_phases(unsigned long long* phases7);
/* LayerNorm absorbed by the Linear that consumes it inside bbbp_mixed_forward (bbbp_layernorm_linear_fwd for norm1 -> linear1 and norm2 -> the
 * next in_proj / fingerprint_fc; dropout + residual move into the producing GEMM's epilogue).  Default 0 (initial value BBBP_LN_ABSORB):
 * built, parity-tested and measured slower inside the B = 512 step.  Returns the previous setting. */
int bbbp_set_ln_absorb(int on);
int bbbp_set_overlap(int on);   /* two/three-stream branch overlap inside bbbp_mixed_forward/backward (default on) */
/* Data-parallel overlap: the gradient of the image-FC weight (62 % of all gradient bytes at F = 167) is final after the
 * first GEMM of the image branch's backward.  wait_bucket(stream, 0) makes `stream` wait for exactly that point of the
 * most recent bbbp_mixed_backward on the current device, so an all-reduce of that bucket can run under the remaining
 * ~2 ms of the backward pass; bucket_param gives the bucket's index in the parameter order.  Bucket 1 = every other
 * gradient except the four conv tensors: final when the fingerprint branch and all weight-gradient leaves are (the image
 * branch's last kernel is then still running); the conv tensors are final only at the end of the pass. */
int bbbp_mixed_backward_wait_bucket(void* stream, int bucket);
/* The same buckets for an OPTIMIZER step pipelined into the pass: `stream` waits until the bucket's gradient slice is final AND the
 * bucket's parameters are no longer read by the most recent bbbp_mixed_backward (bucket 0: after the image FC's input-gradient GEMM;
 * encoder layer l >= 1: when layer l - 1's bucket is final; layer 0 and bucket 1: the end of the fingerprint branch).  The four conv
 * tensors have no bucket: conv2's weight is read by conv2's data gradient, update them after the pass. */
int bbbp_mixed_backward_wait_released(void* stream, int bucket);
/* Bucket 0's release point needs one more event on the image branch's stream: recorded only while this is on (default off).  Returns the
 * previous setting. */
int bbbp_set_release_events(int on);
/* Test hook: the ReLU decisions of encoder layer `layer`'s linear1 (R:75-78; nn.TransformerEncoderLayer.linear1 + ReLU) as
 * the forward pass that filled `workspace` took them -- gate[b * dim_feedforward + j] = 1 where the (post-dropout) hidden
 * activation is > 0.  Parity tests at B = 512 hand these to the float64 oracle: a pre-activation within float32 rounding of
 * zero may legitimately fall on either side, and ONE such element changes that unit's weight-gradient row by percents. */
int bbbp_mixed_debug_ffn_gate(void* stream, const bbbp_mixed_desc* d, const void* workspace, int layer, uint8_t* gate);
/* Test hook, same purpose for the conv stages: the u8 pooling / ReLU decision the forward call saved per POOLED element of stage 1
 * (Conv2d(3,32)+ReLU+MaxPool2d: [B,32,64,64]) or stage 2 (Conv2d(32,64)+...: [B,64,32,32]): 0..3 = position of the first maximum of the
 * 2x2 window in PyTorch's scan order (0,0),(0,1),(1,0),(1,1); 4 = the maximum is <= 0 (ReLU inactive, no gradient).  A window whose
 * two largest pre-activations agree to float32 rounding may legitimately route its gradient to either, and the conv weight / bias
 * gradients are 10^7-term sums over such decisions: B = 512 parity tests hand these to the float64 oracle after checking that they
 * differ from float64's own only at such near-ties. */
int bbbp_mixed_debug_pool_mask(void* stream, const bbbp_mixed_desc* d, const void* workspace, int stage, uint8_t* mask);
int bbbp_mixed_bucket_param(const bbbp_mixed_desc* d, int bucket);
/* Buckets 2 + l (l = encoder layer): the layer's twelve tensors, final when its weight-gradient leaves are (layer L-1 first,
 * layer 0 last).  bucket_range gives first parameter index and tensor count of bucket 0 or 2 + l (consecutive in params[]
 * order, hence one slice of a flat gradient buffer); -1 otherwise. */
int bbbp_mixed_bucket_range(const bbbp_mixed_desc* d, int bucket, int* first, int* count);
/* HIP-graph replay of bbbp_mixed_forward / bbbp_mixed_backward: the second call with identical arguments is captured,
 * later ones are replayed with one hipGraphLaunch.  Opt-in (env BBBP_GRAPHS=1 or bbbp_set_graphs(1), which returns the
 * previous setting): measured slower than the eager three-stream enqueue on ROCm 7.2.  Counters since load. */
int bbbp_set_graphs(int on);
int bbbp_graph_stats(long* captures, long* replays);
int bbbp_profile_enable(int on);
int bbbp_profile_select(unsigned section_mask);   /* bit i = section i records events; 0 = all (the default) */
int bbbp_profile_num_sections(void);
const char* bbbp_profile_section_name(int i);
int bbbp_profile_collect(float* ms_sum, int* count);
/* Before collect(): section id, start and end (ms after the first recorded section's start) of up to max_entries recorded
 * section instances, in recording order; returns how many were written (or a negative error). */
int bbbp_profile_timeline(int* section, float* start_ms, float* end_ms, int max_entries);

#ifdef __cplusplus
}
#endif
#endif /* BBBP_HIP_H */
