// Shared helpers for the gfx950 kernels of the BBBP hot path.  CDNA4 only: wave = 64 lanes.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

#define BBBP_OK 0
#define BBBP_ERR_ARG 1
#define BBBP_ERR_HIP 2
#define BBBP_ERR_WORKSPACE 3

// last-error string, one per host thread (never throws across the C ABI)
void bbbp_set_error(const char* fmt, ...);

#define BBBP_CHECK_ARG(cond, ...)                 \
    do {                                          \
        if (!(cond)) {                            \
            bbbp_set_error(__VA_ARGS__);          \
            return BBBP_ERR_ARG;                  \
        }                                         \
    } while (0)

#define BBBP_CHECK_HIP(expr)                                                            \
    do {                                                                                \
        hipError_t _e = (expr);                                                         \
        if (_e != hipSuccess) {                                                         \
            bbbp_set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
            return BBBP_ERR_HIP;                                                        \
        }                                                                               \
    } while (0)

#define BBBP_CHECK_LAUNCH() BBBP_CHECK_HIP(hipGetLastError())

static inline int cdiv(int a, int b) { return (a + b - 1) / b; }
static inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

int bbbp_num_cus();   // cached multiProcessorCount of the current device
// Grid of a persistent kernel over `nwork` items in runs of `nmb`: `want` work-groups, rounded down to a multiple of 8 * nmb (whole XCD
// rounds, see xcd_adjacent) and capped by the work
static inline int persistent_grid(int want, int nmb, int nwork) {
    int grid = want;
    if (grid >= 8 * nmb) grid -= grid % (8 * nmb);
    if (grid > nwork) grid = nwork - nwork % nmb;
    return grid < nmb ? nmb : grid;
}
int bbbp_ensure_dyn_lds(const void* kernel, size_t bytes);   // hipFuncAttributeMaxDynamicSharedMemorySize once per (kernel, device)
// Opt the kernel in to `lds` bytes of dynamic LDS and launch it.  (hipLaunchKernel, not <<<>>>: a triple-chevron launch inside a header
// template changes the order in which every including file's device variables are emitted.)
template <class P>
int launch_lds(void (*kernel)(P), dim3 grid, int threads, size_t lds, hipStream_t st, const P& p) {
    if (int rc = bbbp_ensure_dyn_lds(reinterpret_cast<const void*>(kernel), lds)) return rc;
    void* args[] = {const_cast<P*>(&p)};
    BBBP_CHECK_HIP(hipLaunchKernel(reinterpret_cast<const void*>(kernel), grid, dim3(threads), args, lds, st));
    return BBBP_OK;
}
// Knobs.  Every BBBP_* environment variable is an integer read through bbbp_env_int (`dflt` when unset); call sites keep the value in a
// `static const`, so it is read once.  bbbp_env is the raw string (NULL when unset) for the one knob that is not parsed as a number.
const char* bbbp_env(const char* name);
int bbbp_env_int(const char* name, int dflt);
static inline int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
// A knob that also has an exported setter: the environment's value at first use, then whatever set() stored.  `norm` is the knob's mask or
// clamp; it is applied to both.
struct Knob {
    const char* env; int dflt; int (*norm)(int);
    int v = -1;
    int get() { if (v < 0) v = norm(bbbp_env_int(env, dflt)); return v; }
    int set(int x) { const int prev = get(); v = norm(x); return prev; }
};
static inline int knob_bool(int v) { return v != 0; }

// CU partitioning for the two-branch overlap (engine.hip).  A persistent conv work-group takes >= 120 KB of a CU's
// 160 KB LDS, so exactly one fits per CU; with `reserved_cus` > 0 the conv grids shrink to (CUs - reserved) and the
// small side-stream kernels request `small_lds_pad` bytes (> 40 KB) so that they can ONLY land on the CUs the conv
// grids left free.  Measured without it: a 5 us kernel sharing CUs with a conv kernel takes 35-85 us.
extern thread_local int g_bbbp_reserved_cus;
extern thread_local size_t g_bbbp_small_lds_pad;
// What a caller wants of a conv stage's kernels: set by the engine from its plan (engine.hip), or from the calling thread's two settable
// values by the C entry points (conv.hip).  conv_choice (conv.hip) weighs them against the BBBP_CONV_WINOGRAD mask and the knobs; the
// measurements behind each field stand there.
struct ConvPrefs {
    int conv1_fwd_f32 = 0;         // keep the first stage's forward on the f32 kernel although the mask selects its split-bf16 form
    int conv1_fwd_per_cu = 0;      // work-groups per CU for the split-bf16 conv1 forward (0 = BBBP_C1_PER_CU)
    int conv2_fwd_pipe = 0;        // forward of the 64 x 64-map stages: the software-pipelined one-work-group-per-CU kernel
    int wgrad_beside_encoder = 0;  // conv2's structured-sparse weight gradient in its 4-wave form (0 = no preference: 8 waves)
};
// Bits of the BBBP_CONV_WINOGRAD mask (bbbp_set_conv_winograd): which stages leave the f32 direct kernels, and for what
enum ConvMaskBit {
    CONV_WINO_FWD = 1, CONV_WINO_DGRAD = 2,                        // conv2 forward / data gradient as Winograd F(2x2,3x3) (conv_wino.hip)
    CONV_B3_FWD = 4, CONV_B3_DGRAD = 8, CONV_B3_WGRAD = 16,        // conv2-family stages as split-bf16 (conv_b3.hip; before the Winograd bits)
    CONV_B3_C1_WGRAD = 32, CONV_B3_C1_FWD = 64,                    // conv1's split-bf16 weight gradient (conv_b3.hip) / forward (conv_b3c1.hip)
    CONV_B3_WGRAD_SPARSE = 128, CONV_B3_WGRAD_SPARSE4 = 256,       // the weight gradient on the 2:4 structured-sparse MFMA / (test hook) its 4-wave form
    CONV_MASK_ALL = 511
};
// The kernel form conv_choice picks for one call; the launchers below receive it decided and decide nothing
enum class ConvForm { F32Direct, Winograd, SplitBf16, SplitBf16Pipe, Conv1SplitBf16, Conv1SplitBf16Pipe, WgradDense, WgradSparse8, WgradSparse4 };
// conv.hip: the C entry points bbbp_conv3x3_relu_pool_fwd / _bwd_weight with the form choices as an argument
int conv3x3_relu_pool_fwd(hipStream_t st, const float* x, const float* w, const float* bias, float* y, uint8_t* mask, int B, int cin, int cout,
                          int H, int W, void* workspace, size_t workspace_bytes, const ConvPrefs& prefs);
int conv3x3_relu_pool_bwd_weight(hipStream_t st, const float* x, const float* gy, const uint8_t* gmask, float* dw, float* dbias, int B, int cin,
                                 int cout, int H, int W, void* workspace, size_t workspace_bytes, const ConvPrefs& prefs);
extern thread_local int g_bbbp_wino_side_cus;      // CUs the Winograd conv grids leave free while the engine overlaps its branches
// head.hip: fused fusion-block + regression-head forward (two launches); `partial`: ceil(B/16) * 2 * 256 floats
int bbbp_head_forward_fused(hipStream_t st, const float* comb, const float* const* fw1, const float* const* fb1,
                            const float* const* fw2, const float* const* fb2, const float* w0, const float* b0, const float* gamma,
                            const float* beta, float* running_mean, float* running_var, const float* w3, const float* b3,
                            const float* w5, const float* b5, const float* w7, const float* b7, float* hid, float* attn, float* fused,
                            float* h, float* hb, float* bn_mean, float* bn_rstd, float* h2, float* h3, float* out, float* partial,
                            int B, int training, int concat);
// head.hip: the input-gradient chain of the head and fusion block backward (two launches); `partial` as above
int bbbp_head_backward_fused(hipStream_t st, const float* dout, const float* comb, const float* hid, const float* attn, const float* h,
                             const float* h2, const float* h3, const float* bn_mean, const float* bn_rstd, const float* gamma,
                             const float* const* fw1, const float* const* fw2, const float* w0, const float* w3, const float* w5,
                             const float* w7, float* dh3, float* dh2, float* dhb, float* dh, float* dlogit, float* dpre, float* dcomb,
                             float* dgamma, float* dbeta, float* partial, int B, int training);
// encoder.hip: the row-local stretches of an encoder layer as single launches (see the file header)
struct bbbp_enc_row_fwd_args {
    const float* ctx; const float* xin;
    const float *wo, *bo, *g1, *be1, *w1, *b1, *w2, *b2, *g2, *be2;
    const float *wn, *bn; float* outn; int nn, ldn, actn;
    float *z1, *y1, *hff, *z2, *y2, *mean1, *rstd1, *mean2, *rstd2;
    int B, F, DFF; float p; uint64_t seed1, seed2, seed3;
};
struct bbbp_enc_row_bwd_args {
    const float* dqkv_up; const float* win_up; const float* dz1_up; float* dyout;
    const float *z2, *mean2, *rstd2, *g2, *w2, *hff, *w1, *z1, *mean1, *rstd1, *g1, *wo;
    float *dz2, *dff, *dhff, *dy1, *dz1, *dsa, *dctx;
    int B, F, DFF; float p; uint64_t seed1, seed3;
};
bool bbbp_enc_rows_supported(int F, int nhead, int dff);
int bbbp_enc_row_fwd(hipStream_t st, const bbbp_enc_row_fwd_args* a);
int bbbp_enc_row_bwd(hipStream_t st, const bbbp_enc_row_bwd_args* a);
int bbbp_ln_param_grad_multi(hipStream_t st, int n, const float* const* dy, const float* const* z, const float* const* mean,
                             const float* const* rstd, float* const* dgamma, float* const* dbeta, int rows, int cols);
// attention.hip: fused (flash-style) self-attention for many heads of head_dim 8 / 16, one work-group per head
bool bbbp_attn_small_supported(int B, int nhead, int head_dim);
bool bbbp_attn_wide_supported(int B, int nhead, int head_dim);      // one wide head (161..176 columns): opt-in, see attention.hip
// `keep` (optional, bbbp_attn_small_keep_bytes): the forward pass leaves its dropout decisions there and the backward pass reads them
// back instead of drawing the Philox blocks again; NULL: backward recomputes them (same stream, same result)
size_t bbbp_attn_small_keep_bytes(int B, int nhead, int head_dim);
int bbbp_attn_small_fwd(hipStream_t st, const float* qkv, float* ctx, float* lse, int B, int F, int nhead, float scale, float p, uint64_t seed,
                        uint8_t* keep = nullptr);
int bbbp_attn_small_bwd(hipStream_t st, const float* qkv, const float* ctx, const float* lse, const float* dctx, float* dqkv, int B, int F,
                        int nhead, float scale, float p, uint64_t seed, const uint8_t* keep = nullptr);
constexpr size_t BBBP_CONV_MIN_LDS = 120 * 1024;
// conv_wino.hip: Winograd F(2x2,3x3) form of the 32 -> 64 @ 64x64 stage; workspace = 16*32*64 floats of transformed filters
int bbbp_wino_conv2_fwd(hipStream_t st, const float* x, const float* w, const float* bias, float* y, uint8_t* mask, int B,
                        float* workspace);
int bbbp_wino_conv2_dgrad(hipStream_t st, const float* gy, const uint8_t* gmask, const float* w, float* dx, int B, float* workspace);
int bbbp_wino_last_clock(unsigned long long* shader_cycles, unsigned long long* ticks_100mhz);
// conv_b3.hip: the same stage as a direct implicit GEMM on the bf16 matrix pipe with every float32 operand split into three bf16
// pieces (six products per float32 product, float32 accumulate); workspace = bbbp_b3_workspace_bytes(cin, cout) of pre-split filters.
// Round 4: the same kernels for the two large stages of the wide / deep variant (64 -> 128 @ 64 x 64, 128 -> 256 @ 32 x 32)
bool bbbp_b3_conv_supported(int cin, int cout, int hw);
size_t bbbp_b3_workspace_bytes(int cin, int cout);
// form: SplitBf16 (per_cu work-groups per CU; probe: the phase-stamping build of the flagship kernel) or SplitBf16Pipe (64 x 64 maps)
int bbbp_b3_conv_fwd(hipStream_t st, const float* x, const float* w, const float* bias, float* y, uint8_t* mask, int B, int cin, int cout, void* workspace,
                     ConvForm form, int per_cu, bool probe);
int bbbp_b3_conv_dgrad(hipStream_t st, const float* gy, const uint8_t* gmask, const float* w, float* dx, int B, int cin, int cout, void* workspace,
                       ConvForm form, int per_cu, bool probe);
// form: WgradDense (64 x 64 maps), WgradSparse8 or WgradSparse4 (64 x 64 or 32 x 32 maps).  cin_total, cout_total: the stage's channel
// counts; groups: work-groups per (32 ci, 64 co) block pair, grid = pairs * groups; map: the stage's map size
int bbbp_b3_conv2_wgrad(hipStream_t st, const float* x, const float* gy, const uint8_t* mask, float* slab, float* bslab, int B, int grid, ConvForm form,
                        int cin_total, int cout_total, int groups, int map);
int bbbp_b3_last_clock(unsigned long long* shader_cycles, unsigned long long* ticks_100mhz);
// conv_b3c1.hip: forward of the first stage (3 -> 32 @ 128x128) in the same arithmetic, channel-innermost LDS strip, no operand assembly.
// form: Conv1SplitBf16Pipe (software-pipelined) or Conv1SplitBf16 (phase by phase), per_cu work-groups per CU
size_t bbbp_b3_conv1_fwd_workspace_bytes();
int bbbp_b3_conv1_fwd(hipStream_t st, const float* x, const float* w, const float* bias, float* y, uint8_t* mask, int B, void* workspace,
                      ConvForm form, int per_cu);
int bbbp_b3_conv1_wgrad(hipStream_t st, const float* x, const float* gy, const uint8_t* mask, float* slab, float* bslab, int B, int grid);
int bbbp_wino_last_phases(unsigned long long* phases4);     // BBBP_WINO_PROBE=1 builds of the kernel only
// rowops.hip: a slice of the optimizer step deferred to a side stream (bbbp_adamw_step_deferred).  Entry points that read parameters
// order themselves behind it: bbbp_param_wait(stream, ptr) waits when ptr lies in the slice (null: unconditionally)
int bbbp_param_wait(hipStream_t st, const void* ptr);
bool bbbp_param_pending_elsewhere(const void* ptr);
// gemm.hip: LayerNorm absorbed by the consuming Linear (bbbp_layernorm_linear_fwd) -- is that the faster form for this product?
bool bbbp_layernorm_linear_preferred(int M, int N, int K);
// fold.hip: out_proj folded into the value projection of a one-head encoder layer (W' = Wo Wv, b' = Wo bv) and the gradients unfolded
bool bbbp_fold_supported(int F, int nhead, int layers);
size_t bbbp_outproj_fold_floats(int F, int which);          // 0 wf [3F][F], 1 bf [3F], 2 wvt [F + 1][F], 3 tdw [F][F], 4 tdb [F]
int bbbp_outproj_fold(hipStream_t st, int layers, int F, const float* const* win, const float* const* bin, const float* const* wo,
                      const float* const* bo, float* const* wf, float* const* bf, float* const* wvt);
int bbbp_outproj_unfold(hipStream_t st, int F, int B, const float* tdw, const float* tdb, const float* wo, const float* wvt, const float* dz,
                        int lddz, float* g_outw, float* g_outb, float* g_inw_v, float* g_inb_v);

// Work-groups are dealt to the 8 XCDs round-robin by id and every XCD has its own L2.  Persistent kernels whose consecutive
// work items share input rows (conv strips and their halos) map group w of n to logical index (w % 8) * (n / 8) + w / 8: the
// groups of one XCD then hold consecutive items at the same time and the shared rows are L2 hits instead of second HBM reads.
__device__ __forceinline__ int xcd_adjacent(int w, int n) { return (n & 7) ? w : (w & 7) * (n >> 3) + (w >> 3); }

// exact f32 MFMA: D[32x32] += A[32x2] * B[2x32]; lane l holds A[l&31][l>>5], B[l>>5][l&31];
// D: col = l&31, row = (r&3) + 8*(r>>2) + 4*(l>>5) for register r of 16.
__device__ __forceinline__ f32x16 mfma32(float a, float b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ int mfma_row(int r, int lane) { return (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5); }

// Split-bf16 arithmetic (conv_b3.hip, gemm.hip): a float is the exact sum of three bf16 pieces hi + mid + lo (3 x 8 significand bits),
// and a product of two floats is, to float32 accuracy, the sum of the six piece products hi*hi, hi*mid, mid*hi, hi*lo, lo*hi, mid*mid --
// six v_mfma_f32_32x32x16_bf16 (f32 accumulate) in place of eight v_mfma_f32_32x32x2_f32, at 2.67x the matrix rate.
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef float f32x2v __attribute__((ext_vector_type(2)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));      // clang vectors stay in registers; arrays of HIP's uint4 struct were demoted to scratch
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
// hi / mid / lo of two floats, packed pairwise (a in the low half).  The residuals are formed with packed-f32 subtractions.
// Range: |x| > 3.3895e38 (the largest bf16, 0x7F7F) rounds to +-inf in the `hi` piece and the residuals become -+inf / NaN: such an
// element poisons its products like an overflow would.  Irrelevant on this path (standardised inputs, weights of order 1, gradients
// far below 1e38) -- stated so that nobody re-uses the split on unscaled data without a clamp.  NaN stays NaN, +-inf stays +-inf in
// `hi` (v_cvt_pk_bf16_f32) with NaN residuals.
__device__ __forceinline__ void split2(float a, float b, uint32_t& hi, uint32_t& mid, uint32_t& lo) {
    f32x2v v = {a, b};
    bf16x2 h = __builtin_convertvector(v, bf16x2);
    hi = __builtin_bit_cast(uint32_t, h);
    f32x2v hf = {__builtin_bit_cast(float, hi << 16), __builtin_bit_cast(float, hi & 0xffff0000u)};
    v = v - hf;
    bf16x2 m = __builtin_convertvector(v, bf16x2);
    mid = __builtin_bit_cast(uint32_t, m);
    f32x2v mf = {__builtin_bit_cast(float, mid << 16), __builtin_bit_cast(float, mid & 0xffff0000u)};
    v = v - mf;
    bf16x2 l = __builtin_convertvector(v, bf16x2);
    lo = __builtin_bit_cast(uint32_t, l);
}

// Philox-4x32-10 counter RNG for dropout masks (recomputed, never stored)
__device__ __forceinline__ uint4 philox4(uint64_t seed, uint64_t ctr) {
    uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
    uint32_t c0 = (uint32_t)ctr, c1 = (uint32_t)(ctr >> 32), c2 = 0x9E3779B9u, c3 = 0xBB67AE85u;
#pragma unroll
    for (int i = 0; i < 10; ++i) {
        uint64_t p0 = (uint64_t)0xD2511F53u * c0;
        uint64_t p1 = (uint64_t)0xCD9E8D57u * c2;
        uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0;
        uint32_t n1 = (uint32_t)p1;
        uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        uint32_t n3 = (uint32_t)p0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    return make_uint4(c0, c1, c2, c3);
}
// The engine keeps the per-call dropout seed in DEVICE memory (a slot of the forward workspace, written by a one-thread
// kernel) so that the enqueued work does not depend on it and can be replayed as a HIP graph; kernels then receive the
// slot's address in `base` and a per-site salt in `seed`.  The op-level C entry points pass base = nullptr.
extern thread_local const unsigned long long* g_bbbp_seed_base;
__device__ __forceinline__ uint64_t effective_seed(uint64_t seed, const unsigned long long* base) {
    return base ? (uint64_t)(*base) * 0x9E3779B97F4A7C15ull + seed : seed;
}
// keep-scale for element `idx` of dropout stream `seed`: 0 or 1/(1-p)
__device__ __forceinline__ float dropout_scale(uint64_t seed, uint64_t idx, float p, float inv_keep) {
    uint4 r = philox4(seed, idx >> 2);
    uint32_t v = (idx & 3) == 0 ? r.x : (idx & 3) == 1 ? r.y : (idx & 3) == 2 ? r.z : r.w;
    // uniform in [0,1): top 24 bits
    float u = (float)(v >> 8) * (1.0f / 16777216.0f);
    return u >= p ? inv_keep : 0.0f;
}

// Small latency-bound kernels run beside persistent MFMA-bound conv work-groups (engine.hip, two streams); raising
// their wave priority lets them win issue arbitration against the older conv waves on the same SIMD.
#ifndef BBBP_HIGH_PRIO
#define BBBP_HIGH_PRIO() __builtin_amdgcn_s_setprio(3)
#endif
