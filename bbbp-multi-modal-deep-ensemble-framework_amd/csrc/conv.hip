// 3x3 / stride 1 / pad 1 convolution fused with ReLU and 2x2 max-pool, forward and backward, as
// implicit GEMMs on the exact-f32 MFMA (v_mfma_f32_32x32x2_f32) for gfx950.
//
// Replaces `nn.Conv2d(k=3,s=1,p=1) -> nn.ReLU -> nn.MaxPool2d(2,2)` of the reference's image branch
// (Models/multi_input_data_regression_opt_transformer_cnn_20250113.py:84-90) and
// their autograd backward (a12).  NCHW fp32 in and out, exactly the reference's tensor layout.
//
// Forward / data-gradient kernel (one template):
//   GEMM view  D[co][pixel] = sum_{tap,ci} Wt[tap][ci][co] * X[ci][pixel shifted by tap]
//   M = output channels (MFMA rows), N = 32 consecutive pixels of one image row (MFMA columns, so
//   a half-wave reads 32 consecutive floats of the LDS strip: conflict-free), K = (tap, ci) with
//   ci fastest, so the two k of one MFMA are two adjacent channel planes (a constant LDS delta).
//   A work-group owns a strip of TH output rows x the full width of one image; each of its 8 waves
//   owns 2 rows x 32 columns x all output channels, so the 2x2 pool partners are the wave's two
//   accumulator tiles (rows) and the neighbouring lane (columns, one DPP shuffle).  Weights
//   (pre-transposed to [tap][ci][co] by a prep kernel) stay resident in LDS; input channels stream
//   through a double-buffered LDS strip in chunks of 8 (register-staged prefetch under the MFMAs).
//   MODE_FWD:   + bias, ReLU, max-pool; writes pooled y and a u8 mask (argmax 0..3 in PyTorch's
//               first-max order, 4 = ReLU inactive) that backward uses instead of the 4x larger
//               pre-pool activation.
//   MODE_DGRAD: the strip loader expands the pooled gradient through the mask on the fly
//               (dYfull is never materialised); the prep kernel flips/transposes the weights.
// Weight-gradient kernels: D[co][(tap,ci)] = sum_pixels dYfull[co][pixel] * X[ci][pixel + tap],
//   K = pixels; each work-group reduces its waves' K-partials in LDS, writes one partial slab, and a
//   second kernel sums the slabs in a fixed order (bit-reproducible; no float atomics).
#include "common.h"
#include "bbbp_hip.h"
#include <limits.h>
#include <algorithm>
#include <stdlib.h>

namespace {

constexpr int MODE_FWD = 0;
constexpr int MODE_DGRAD = 1;
constexpr int PADL = 4;           // left halo column sits at index PADL-1 so data columns are 16-B aligned

struct ConvParams {
    const float* x;        // FWD: input [B][CIN][H][W];  DGRAD: pooled grad [B][CIN][H/2][W/2]
    const uint8_t* xmask;  // DGRAD: mask of the pooled grad
    const float* wt;       // prepped weights [9][CINP][COUT]
    const float* bias;     // FWD: [COUT]
    float* y;              // FWD: pooled [B][COUT][H/2][W/2];  DGRAD: [B][COUT][H][W]
    uint8_t* ymask;        // FWD: [B][COUT][H/2][W/2]
    int B, H;
    int co_total;          // all output channels; the kernel computes COUT of them per work item (block cb)
};

template <int CIN, int COUT, int W, int MODE>
struct ConvCfg {
    static constexpr int NW = 4;                             // waves per work-group (one per SIMD)
    static constexpr int NT = NW * 64;
    static constexpr int CC = 4;                              // channels per LDS stage (8 measured equal; 4 halves the LDS footprint)
    static constexpr int NCH = (CIN + CC - 1) / CC;
    static constexpr int CINP = NCH * CC;
    static constexpr int TH = NT / W;                        // strip rows: NW wave tiles of 2 rows x 32 columns
    static constexpr int ROWS = TH + 2;
    static constexpr int LDW = W + 8;
    static constexpr int PLANE = ROWS * LDW;
    static constexpr int XCHUNK = CC * PLANE;                // input floats per stage
    static constexpr int WCHUNK = 9 * CC * COUT;             // weight floats per stage: [tap][ci in chunk][co]
    static constexpr bool WRES = (NCH == 1);                 // a single chunk: weights stay resident
    static constexpr int STAGE = XCHUNK + (WRES ? 0 : WCHUNK);
    static constexpr int MT = COUT / 32;
    static constexpr size_t LDS_BYTES = (size_t)(2 * STAGE + (WRES ? WCHUNK : 0)) * sizeof(float);
    static_assert(COUT % 32 == 0 && MT <= 2, "output channels: 32 or 64 per pass");
    static_assert(TH >= 2 && TH % 2 == 0 && W % 32 == 0, "tile shape");
    static_assert(CC % 2 == 0, "k pairs are adjacent channel planes");
};

// swap with the neighbouring lane (lane ^ 1) in one VALU op (DPP quad_perm [1,0,3,2])
__device__ __forceinline__ float swap_lane1(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0xB1, 0xF, 0xF, false));
}

// Shader-clock cycles and 100 MHz wall ticks spent by work-group 0 of the last forward / data-gradient launch (it is
// persistent, so that is very nearly the launch).  bench.py derives the SUSTAINED clock and the matrix-pipe occupancy
// from it: under a chip-wide f32 MFMA stream the clock settles near 2.3 GHz, below the 2.4 GHz of the quoted peak.
__device__ unsigned long long g_conv_clock[2];

template <int CIN, int COUT, int W, int MODE>
__global__ __launch_bounds__(256, 2) void conv3x3_kernel(ConvParams p) {
    using C = ConvCfg<CIN, COUT, W, MODE>;
    const unsigned long long clk0 = __builtin_readcyclecounter(), wall0 = wall_clock64();
    constexpr int NT = C::NT, CC = C::CC, NCH = C::NCH, CINP = C::CINP, TH = C::TH, ROWS = C::ROWS, LDW = C::LDW,
                  PLANE = C::PLANE, XCHUNK = C::XCHUNK, WCHUNK = C::WCHUNK, STAGE = C::STAGE, MT = C::MT;
    constexpr bool WRES = C::WRES;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    // stage s: [X chunk][W chunk]; resident weights (single-chunk layers) sit behind the two stages
    float* Wres = smem + 2 * STAGE;

    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int H = p.H;
    const int strips_per_img = H / TH;
    const int ncb = p.co_total / COUT;                        // output-channel blocks; work item = (strip, block)
    const int nstrips = p.B * strips_per_img * ncb;           // (named nstrips for history: number of work items)
    const int CO_T = p.co_total;

    // zero both input stages once: halo columns and padded channel planes are never written again
    for (int s = 0; s < 2; ++s)
        for (int i = t * 4; i < XCHUNK; i += NT * 4)
            *reinterpret_cast<float4*>(smem + s * STAGE + i) = make_float4(0.f, 0.f, 0.f, 0.f);
    if (WRES)
        for (int i = t * 4; i < WCHUNK; i += NT * 4)
            *reinterpret_cast<float4*>(Wres + i) = *reinterpret_cast<const float4*>(p.wt + i);
    __syncthreads();

    // ---- stage loader (register staged): input strip chunk + (streamed) weight chunk ----
    constexpr int QW = (MODE == MODE_FWD) ? W / 4 : W / 8;      // work items per row
    constexpr int LCH = CIN < CC ? CIN : CC;                    // planes actually staged (the 4th plane of an RGB input stays zero)
    constexpr int ITEMS = LCH * ROWS * QW;
    constexpr int NIT = (ITEMS + NT - 1) / NT;
    constexpr int WQ = WRES ? 0 : WCHUNK / 4;                   // float4 of weights per stage
    constexpr int WNIT = (WQ + NT - 1) / NT;
    float4 rg[NIT];
    uint32_t rm[NIT];
    f32x4 rw[WNIT > 0 ? WNIT : 1];     // clang vector type: the float4 struct array was demoted to scratch here
    uint32_t okbits = 0;       // validity of the staged items (bit i), applied when they are written to LDS
    // NOTE: every load below is UNCONDITIONAL (addresses are clamped into the tensor).  A load under a per-item
    // `if` makes hipcc wait vmcnt(0) at the join, which exposed the full HBM latency once per stage.
    auto load_stage = [&](int work, int chunk) __attribute__((always_inline)) {
        const int strip = work / ncb, cb = work % ncb;
        const int b = strip / strips_per_img, h0 = (strip % strips_per_img) * TH;
        okbits = 0;
#pragma unroll
        for (int i = 0; i < NIT; ++i) {
            int idx = t + i * NT;
            int q = idx % QW, row = (idx / QW) % ROWS, ci = idx / (QW * ROWS);
            int c = chunk * CC + ci, hh = h0 - 1 + row;
            bool ok = idx < ITEMS && c < CIN && hh >= 0 && hh < H;
            okbits |= (ok ? 1u : 0u) << i;
            int cc = min(c, CIN - 1), hc = min(max(hh, 0), H - 1);
            if (MODE == MODE_FWD) {
                rg[i] = *reinterpret_cast<const float4*>(p.x + (((long)b * CIN + cc) * H + hc) * W + q * 4);
            } else {
                long off = (((long)b * CIN + cc) * (H / 2) + (hc >> 1)) * (W / 2) + q * 4;
                rg[i] = *reinterpret_cast<const float4*>(p.x + off);
                rm[i] = *reinterpret_cast<const uint32_t*>(p.xmask + off);
            }
        }
        if (!WRES) {
#pragma unroll
            for (int i = 0; i < WNIT; ++i) {
                int idx = min(t + i * NT, WQ - 1);           // float4 index within [tap][CC][COUT]
                int tap = idx / (CC * COUT / 4), rem = idx % (CC * COUT / 4);
                int cil = rem / (COUT / 4), q4 = rem % (COUT / 4);
                rw[i] = *reinterpret_cast<const f32x4*>(p.wt + ((long)tap * CINP + chunk * CC + cil) * CO_T + cb * COUT + q4 * 4);
            }
        }
    };
    auto store_stage = [&](int work, int buf) __attribute__((always_inline)) {
        const int h0 = ((work / ncb) % strips_per_img) * TH;
        float* xs = smem + buf * STAGE;
#pragma unroll
        for (int i = 0; i < NIT; ++i) {
            int idx = t + i * NT;
            if (idx >= ITEMS) continue;
            int q = idx % QW, row = (idx / QW) % ROWS, ci = idx / (QW * ROWS);
            const bool ok = (okbits >> i) & 1u;
            if (MODE == MODE_FWD) {
                float4 v = rg[i];
                v.x = ok ? v.x : 0.f; v.y = ok ? v.y : 0.f; v.z = ok ? v.z : 0.f; v.w = ok ? v.w : 0.f;
                *reinterpret_cast<float4*>(xs + ci * PLANE + row * LDW + PADL + q * 4) = v;
            } else {
                // expand 4 pooled gradients to the 8 full-resolution columns of image row hh
                int pr = ((h0 - 1 + row) & 1) * 2;     // (hh & 1) also for hh = -1 (two's complement)
                uint32_t m = ok ? rm[i] : 0x04040404u;
                float4 lo, hi;
                lo.x = ((m & 0xff) == (uint32_t)pr) ? rg[i].x : 0.f;
                lo.y = ((m & 0xff) == (uint32_t)pr + 1) ? rg[i].x : 0.f;
                lo.z = (((m >> 8) & 0xff) == (uint32_t)pr) ? rg[i].y : 0.f;
                lo.w = (((m >> 8) & 0xff) == (uint32_t)pr + 1) ? rg[i].y : 0.f;
                hi.x = (((m >> 16) & 0xff) == (uint32_t)pr) ? rg[i].z : 0.f;
                hi.y = (((m >> 16) & 0xff) == (uint32_t)pr + 1) ? rg[i].z : 0.f;
                hi.z = ((m >> 24) == (uint32_t)pr) ? rg[i].w : 0.f;
                hi.w = ((m >> 24) == (uint32_t)pr + 1) ? rg[i].w : 0.f;
                float* d = xs + ci * PLANE + row * LDW + PADL + q * 8;
                *reinterpret_cast<float4*>(d) = lo;
                *reinterpret_cast<float4*>(d + 4) = hi;
            }
        }
        if (!WRES) {
            float* wsd = xs + XCHUNK;
#pragma unroll
            for (int i = 0; i < WNIT; ++i) {
                int idx = t + i * NT;
                if (idx < WQ) *reinterpret_cast<f32x4*>(wsd + idx * 4) = rw[i];
            }
        }
    };

    // wave tile: row pair rp, 32-column segment seg
    constexpr int SEGS = W / 32;
    const int rp = wave / SEGS, seg = wave % SEGS;
    const int r0 = 2 * rp, c0 = seg * 32;
    const int j = lane & 31, kh2 = lane >> 5;
    const int xbase = kh2 * PLANE + r0 * LDW + c0 + j + PADL - 1;
    const int wbase = kh2 * COUT + j;

    // CIN = 3: per-lane offsets of the flattened K walk; k = 2 * step + (lane >> 5), row of Wt[tap][4][co] and LDS offset
    int koff_w[14], koff_x[14];
    if (CIN == 3) {
#pragma unroll
        for (int st = 0; st < 14; ++st) {
            const int k = 2 * st + kh2;
            const int tap = k < 27 ? k / 3 : 0, ci = k < 27 ? k % 3 : 3;          // k = 27: the zero row (tap 0, plane 3)
            koff_w[st] = (tap * CC + ci) * COUT;
            koff_x[st] = ci * PLANE + (tap / 3) * LDW + (tap % 3);
        }
    }

    f32x16 acc[MT][2];

    int strip = xcd_adjacent(blockIdx.x, gridDim.x);
    if (strip < nstrips) {
        load_stage(strip, 0);
        store_stage(strip, 0);
    }
    __syncthreads();
    int buf = 0;
    for (; strip < nstrips; strip += gridDim.x) {
        const int cb = strip % ncb;
        const int b = (strip / ncb) / strips_per_img, h0 = ((strip / ncb) % strips_per_img) * TH;
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                float bv = 0.f;
                if (MODE == MODE_FWD) bv = p.bias[cb * COUT + mt * 32 + mfma_row(r, lane)];
                acc[mt][0][r] = bv;
                acc[mt][1][r] = bv;
            }
        }
        for (int chunk = 0; chunk < NCH; ++chunk) {
            // prefetch the next stage into registers
            int nstrip = strip, nchunk = chunk + 1;
            if (nchunk == NCH) { nchunk = 0; nstrip = strip + gridDim.x; }
            const bool have_next = nstrip < nstrips;
            if (have_next) load_stage(nstrip, nchunk);

            const float* xs = smem + buf * STAGE + xbase;
            const float* ws = (WRES ? Wres : smem + buf * STAGE + XCHUNK) + wbase;
            const float* xs3 = smem + buf * STAGE + r0 * LDW + c0 + j + PADL - 1;      // CIN = 3: the k half is in koff_x
            const float* ws3 = Wres + j;
            // 9 taps x CC/2 channel pairs = NS k-steps, software pipelined: the LDS reads of step s+1 are issued
            // BEFORE the MFMAs of step s (hipcc otherwise issues them after, exposing the LDS latency every step).
            // RGB input (CIN = 3): K = 27 is walked flat, k = tap * 3 + ci, 14 steps instead of 9 x 2 = 18 over a
            // zero-padded 4th plane; the two k of a step are then different (tap, ci) pairs, so each lane keeps its
            // 14 weight-row and 14 input offsets in registers (koff_w / koff_x, set up once before the strip loop).
            constexpr int NS = (CIN == 3) ? 14 : 9 * (CC / 2);
            float a[2][MT], bb[2][2];
            auto ld = [&](int st, float* av, float* bv) __attribute__((always_inline)) {
                if constexpr (CIN == 3) {
#pragma unroll
                    for (int mt = 0; mt < MT; ++mt) av[mt] = ws3[koff_w[st] + mt * 32];
#pragma unroll
                    for (int n = 0; n < 2; ++n) bv[n] = xs3[koff_x[st] + n * LDW];
                } else {
                    const int tap = st / (CC / 2), cp = st % (CC / 2), kh = tap / 3, kw = tap % 3;
#pragma unroll
                    for (int mt = 0; mt < MT; ++mt) av[mt] = ws[(tap * CC + 2 * cp) * COUT + mt * 32];
#pragma unroll
                    for (int n = 0; n < 2; ++n) bv[n] = xs[(2 * cp) * PLANE + (n + kh) * LDW + kw];
                }
            };
            ld(0, a[0], bb[0]);
#pragma unroll
            for (int st = 0; st < NS; ++st) {
                if (st + 1 < NS) ld(st + 1, a[(st + 1) & 1], bb[(st + 1) & 1]);
#pragma unroll
                for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                    for (int n = 0; n < 2; ++n) acc[mt][n] = mfma32(a[st & 1][mt], bb[st & 1][n], acc[mt][n]);
                __builtin_amdgcn_sched_group_barrier(0x100, MT + 2, 0);     // DS reads of the next step first
                __builtin_amdgcn_sched_group_barrier(0x008, MT * 2, 0);     // then this step's MFMAs
            }
            if (have_next) store_stage(nstrip, buf ^ 1);
            __syncthreads();
            buf ^= 1;
        }
        // ---- epilogue ----
        if (MODE == MODE_FWD) {
            // 2x2 max-pool: rows are the wave's two accumulator tiles, columns are lane pairs (2w, 2w+1).  Even lanes
            // finish register r, odd lanes register r+1, so every lane stores: one DPP swap per value, half the stores.
            const int ph = (h0 + r0) >> 1, Hp = H / 2, Wp = W / 2;
            const bool odd = j & 1;
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) {
#pragma unroll
                for (int r = 0; r < 16; r += 2) {
                    float a0 = acc[mt][0][r], a1 = acc[mt][0][r + 1];     // image row h:   registers r, r+1
                    float b0 = acc[mt][1][r], b1 = acc[mt][1][r + 1];     // image row h+1
                    float ra = swap_lane1(odd ? a0 : a1);                 // even gets odd's a0, odd gets even's a1
                    float rb = swap_lane1(odd ? b0 : b1);
                    float v00 = odd ? ra : a0, v01 = odd ? a1 : ra;
                    float v10 = odd ? rb : b0, v11 = odd ? b1 : rb;
                    // PyTorch max-pool keeps the FIRST maximum in (h, w) scan order
                    float m = v00; int am = 0;
                    if (v01 > m) { m = v01; am = 1; }
                    if (v10 > m) { m = v10; am = 2; }
                    if (v11 > m) { m = v11; am = 3; }
                    int co = cb * COUT + mt * 32 + mfma_row(r + (odd ? 1 : 0), lane);
                    long o = (((long)b * CO_T + co) * Hp + ph) * Wp + ((c0 + j) >> 1);
                    p.y[o] = m > 0.f ? m : 0.f;
                    if (p.ymask) p.ymask[o] = m > 0.f ? (uint8_t)am : (uint8_t)4;       // null: a forward-only plan keeps no decisions
                }
            }
        } else {
#pragma unroll
            for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                for (int n = 0; n < 2; ++n)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        int co = cb * COUT + mt * 32 + mfma_row(r, lane);
                        p.y[(((long)b * CO_T + co) * H + h0 + r0 + n) * W + c0 + j] = acc[mt][n][r];
                    }
        }
    }
    if (blockIdx.x == 0 && t == 0) {
        g_conv_clock[0] = __builtin_readcyclecounter() - clk0;
        g_conv_clock[1] = wall_clock64() - wall0;
    }
}

// Wt[tap][ci][co] from the reference layout W[co][ci][kh][kw].
//  FWD   : Wt[tap][ci][co]      = W[co][ci][tap]                       (CINP >= CIN zero padded)
//  DGRAD : Wt[tap][c=co][o=ci]  = W[co][ci][8 - tap]   (kernel flipped, channel roles swapped)
__global__ void conv_prep_weights_kernel(const float* w, float* wt, int cin, int cout, int cinp_fwd, int mode) {
    int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (mode == MODE_FWD) {
        int total = 9 * cinp_fwd * cout;
        if (idx >= total) return;
        int co = idx % cout, ci = (idx / cout) % cinp_fwd, tap = idx / (cout * cinp_fwd);
        wt[idx] = ci < cin ? w[((long)co * cin + ci) * 9 + tap] : 0.f;
    } else {
        int total = 9 * cout * cin;     // [tap][cout as input channel][cin as output channel]
        if (idx >= total) return;
        int o = idx % cin, c = (idx / cin) % cout, tap = idx / (cin * cout);
        wt[idx] = w[((long)c * cin + o) * 9 + (8 - tap)];
    }
}

// ------------------------------------------------------------------------------------------------
// weight gradient, CIN = 32: M = co (COUT/32 tiles), N = (tap, ci) 9 tiles of 32, K = pixels.
// waves: mt = wave % MT, kg = wave / MT; a strip is 2 output rows; each k-group owns 256/KG... pixels
// ------------------------------------------------------------------------------------------------
struct WgradParams {
    const float* x;        // layer input [B][CIN][H][W]
    const float* gy;       // pooled output gradient [B][COUT][H/2][W/2]
    const uint8_t* mask;   // [B][COUT][H/2][W/2]
    float* slab;           // [grid][COUT][9*32]  (CIN = 32)  or [grid][32][32] (CIN = 3)
    float* bslab;          // [grid][COUT] bias-gradient partials
    int B, H;
    int cin_total, cout_total;   // the kernel handles one (32-input-channel, COUT-output-channel) block pair per work-group
    int groups;                  // work-groups per pair: blockIdx.x = pair * groups + g
};

template <int COUT, int W>
struct WgCfg {
    static constexpr int CIN = 32;
    static constexpr int MT = COUT / 32;
    static constexpr int KG = 8 / MT;                // k-groups of waves
    static constexpr int NPIX = 2 * W;               // pixels per strip (2 rows)
    static constexpr int LDP = NPIX + 1;             // dY row stride: = 1 mod 32 -> conflict-free
    static constexpr int LDW = W + 8;
    static constexpr int PLANE = 4 * LDW + 1;        // odd: lanes = channels hit distinct banks
    static constexpr int DYF = COUT * LDP;
    static constexpr int XF = CIN * PLANE;
    static constexpr int BUF = DYF + XF;
    static constexpr size_t LDS_BYTES = (size_t)2 * BUF * sizeof(float);
    static constexpr int PIX_PER_KG = NPIX / KG;
    static_assert(NPIX % KG == 0 && PIX_PER_KG % 2 == 0 && W % PIX_PER_KG == 0, "k-group split");
};

// Channel totals are template constants: with run-time strides the kernel needs 228 VGPRs instead of 224, and 224 x 2 waves
// per SIMD is what leaves 64 registers per lane free for the side-stream kernels' waves (measured: at 232 the
// fingerprint chain beside this kernel ran 7 % longer).
template <int COUT, int W, int CIN_TOTAL, int COUT_TOTAL>
__global__ __launch_bounds__(512) void conv_wgrad32_kernel(WgradParams p) {
    using C = WgCfg<COUT, W>;
    constexpr int CIN = 32, MT = C::MT, KG = C::KG, LDP = C::LDP, LDW = C::LDW, PLANE = C::PLANE;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int H = p.H, Hp = H / 2, Wp = W / 2;
    const int strips_per_img = H / 2;
    const int nstrips = p.B * strips_per_img;
    const int pair = blockIdx.x / p.groups, grp = blockIdx.x % p.groups;
    constexpr int ncib = CIN_TOTAL / 32;
    const int cob = pair / ncib, cib = pair % ncib;          // output / input channel block of this work-group
    constexpr int CIN_T = CIN_TOTAL, COUT_T = COUT_TOTAL;
    // block offsets folded into the (wave-uniform) base pointers: per-thread address math stays as in the single-pair case
    const float* xbase = p.x + (long)cib * 32 * H * W;
    const float* gybase = p.gy + (long)cob * COUT * Hp * Wp;
    const uint8_t* mbase = p.mask + (long)cob * COUT * Hp * Wp;

    for (int i = t; i < 2 * C::BUF; i += 512) smem[i] = 0.f;
    __syncthreads();

    // loader: dY items (co, q4): COUT * (Wp/4); X items (ci, row, q): 32 * 4 * (W/4)
    constexpr int DY_ITEMS = COUT * (Wp / 4);
    constexpr int DY_NIT = (DY_ITEMS + 511) / 512;
    constexpr int X_ITEMS = CIN * 4 * (W / 4);
    constexpr int X_NIT = (X_ITEMS + 511) / 512;
    float4 gq[DY_NIT]; uint32_t mq[DY_NIT]; float4 xq[X_NIT];
    float bsum[DY_NIT];      // bias-gradient partial of this thread's fixed channel
#pragma unroll
    for (int i = 0; i < DY_NIT; ++i) bsum[i] = 0.f;
    auto load_stage = [&](int strip) __attribute__((always_inline)) {
        const int b = strip / strips_per_img, ph = strip % strips_per_img, h0 = ph * 2;
        // unconditional loads from clamped addresses (a load under a per-item `if` makes hipcc wait vmcnt(0) at the
        // join and exposes the HBM latency every strip); out-of-range items are zeroed with selects afterwards
#pragma unroll
        for (int i = 0; i < DY_NIT; ++i) {
            int idx = min(t + i * 512, DY_ITEMS - 1);
            int q = idx % (Wp / 4), co = idx / (Wp / 4);
            long off = (((long)b * COUT_T + co) * Hp + ph) * Wp + q * 4;
            gq[i] = *reinterpret_cast<const float4*>(gybase + off);
            mq[i] = *reinterpret_cast<const uint32_t*>(mbase + off);
        }
#pragma unroll
        for (int i = 0; i < X_NIT; ++i) {
            int idx = min(t + i * 512, X_ITEMS - 1);
            int q = idx % (W / 4), row = (idx / (W / 4)) % 4, ci = idx / (W / 4 * 4);
            int hh = h0 - 1 + row;
            const bool ok = hh >= 0 && hh < H;
            float4 v = *reinterpret_cast<const float4*>(xbase + (((long)b * CIN_T + ci) * H + min(max(hh, 0), H - 1)) * W + q * 4);
            xq[i].x = ok ? v.x : 0.f; xq[i].y = ok ? v.y : 0.f; xq[i].z = ok ? v.z : 0.f; xq[i].w = ok ? v.w : 0.f;
        }
    };
    auto store_stage = [&](int buf) __attribute__((always_inline)) {
        float* dys = smem + buf * C::BUF;
        float* xs = dys + C::DYF;
#pragma unroll
        for (int i = 0; i < DY_NIT; ++i) {
            int idx = t + i * 512;
            if (idx >= DY_ITEMS) continue;
            int q = idx % (Wp / 4), co = idx / (Wp / 4);
            float* d = dys + co * LDP + q * 8;
            float g[4] = {gq[i].x, gq[i].y, gq[i].z, gq[i].w};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                uint32_t m = (mq[i] >> (8 * e)) & 0xff;
                bsum[i] += m < 4 ? g[e] : 0.f;
                d[2 * e] = m == 0 ? g[e] : 0.f;
                d[2 * e + 1] = m == 1 ? g[e] : 0.f;
                d[W + 2 * e] = m == 2 ? g[e] : 0.f;
                d[W + 2 * e + 1] = m == 3 ? g[e] : 0.f;
            }
        }
#pragma unroll
        for (int i = 0; i < X_NIT; ++i) {
            int idx = t + i * 512;
            if (idx >= X_ITEMS) continue;
            int q = idx % (W / 4), row = (idx / (W / 4)) % 4, ci = idx / (W / 4 * 4);
            float* d = xs + ci * PLANE + row * LDW + PADL + q * 4;
            d[0] = xq[i].x; d[1] = xq[i].y; d[2] = xq[i].z; d[3] = xq[i].w;
        }
    };

    const int mt = wave % MT, kg = wave / MT;
    const int pix0 = kg * C::PIX_PER_KG;                 // first pixel of this k-group in the strip
    const int prow = pix0 / W, pcol = pix0 % W;
    const int j = lane & 31, k2 = lane >> 5;
    const int abase = (mt * 32 + j) * LDP + pix0 + k2;
    const int bbase = j * PLANE + prow * LDW + pcol + k2 + PADL - 1;

    f32x16 acc[9];
#pragma unroll
    for (int i = 0; i < 9; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;

    int strip = xcd_adjacent(grp, p.groups);       // groups % 8 == 0 keeps id % 8 == grp % 8 for every (channel block) pair; else identity
    if (strip < nstrips) { load_stage(strip); store_stage(0); }
    __syncthreads();
    int buf = 0;
    for (; strip < nstrips; strip += p.groups) {
        const int nstrip = strip + p.groups;
        if (nstrip < nstrips) load_stage(nstrip);
        const float* dys = smem + buf * C::BUF + abase;
        const float* xs = smem + buf * C::BUF + C::DYF + bbase;
#pragma unroll 4
        for (int pp = 0; pp < C::PIX_PER_KG; pp += 2) {
            float a = dys[pp];
#pragma unroll
            for (int tap = 0; tap < 9; ++tap) {
                float bv = xs[(tap / 3) * LDW + (tap % 3) + pp];
                acc[tap] = mfma32(a, bv, acc[tap]);
            }
        }
        if (nstrip < nstrips) store_stage(buf ^ 1);
        __syncthreads();
        buf ^= 1;
    }
    // reduce the k-groups through LDS (staging buffers are free now): group g -> LDS, group 0 adds
    float* red = smem;     // MT * 9 * 1024 floats <= 2*BUF
    for (int g = 1; g < KG; ++g) {
        if (kg == g) {
#pragma unroll
            for (int tap = 0; tap < 9; ++tap)
#pragma unroll
                for (int r = 0; r < 16; ++r) red[((mt * 9 + tap) * 16 + r) * 64 + lane] = acc[tap][r];
        }
        __syncthreads();
        if (kg == 0) {
#pragma unroll
            for (int tap = 0; tap < 9; ++tap)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[tap][r] += red[((mt * 9 + tap) * 16 + r) * 64 + lane];
        }
        __syncthreads();
    }
    // bias-gradient partials: the Wp/4 consecutive lanes of one channel reduce by shuffles
#pragma unroll
    for (int i = 0; i < DY_NIT; ++i) {
        float v = bsum[i];
#pragma unroll
        for (int o = 1; o < Wp / 4; o <<= 1) v += __shfl_xor(v, o);
        int idx = t + i * 512;
        if (idx < DY_ITEMS && idx % (Wp / 4) == 0) p.bslab[(long)blockIdx.x * COUT + idx / (Wp / 4)] = v;
    }
    if (kg == 0) {
        float* s = p.slab + (long)blockIdx.x * COUT * 288;
#pragma unroll
        for (int tap = 0; tap < 9; ++tap)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                int co = mt * 32 + mfma_row(r, lane);
                s[co * 288 + tap * 32 + j] = acc[tap][r];
            }
    }
}

// dW[cob*64+co][cib*32+ci][tap] = sum_g slab[pair][g][co][tap*32+ci]; db[cob*64+co] = sum_g bslab[pair(cib=0)][g][co]
// grid: (ceil((64*288 + 64) / 64), pairs).  Fixed summation order.
// sum of slab[g * stride] for g in [g0, g1), 8 independent loads in flight, added in slab order
__device__ __forceinline__ float slab_sum(const float* slab, long stride, int g0, int g1) {
    float s = 0.f;
    int g = g0;
    for (; g + 8 <= g1; g += 8) {
        float v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = slab[(long)(g + u) * stride];
#pragma unroll
        for (int u = 0; u < 8; ++u) s += v[u];
    }
    for (; g < g1; ++g) s += slab[(long)g * stride];
    return s;
}

__global__ __launch_bounds__(1024) void conv_wgrad32_reduce_kernel(const float* slab, const float* bslab, float* dw,
                                                                 float* db, int groups, int cin_total, int cout_total) {
    // 16 thread groups each sum a contiguous range of slabs (few, independent loads per thread: the old 4-group version
    // was a chain of 64 dependent-latency loads and took 19 us for 19 MB), then one group adds the 16 partials in order
    __shared__ float part[16][64];
    constexpr int CO = 64, total = CO * 288;
    const int pair = blockIdx.y, ncib = cin_total / 32, cob = pair / ncib, cib = pair % ncib;
    const int nl = threadIdx.x & 63, grp = threadIdx.x >> 6;
    const int n = blockIdx.x * 64 + nl;          // [0, total) weights, [total, total + CO) biases
    float s = 0.f;
    int per = (groups + 15) / 16;
    int g0 = min(groups, grp * per), g1 = min(groups, g0 + per);
    const float* sl = slab + (long)pair * groups * total;
    const float* bs = bslab + (long)pair * groups * CO;
    if (n < total) s = slab_sum(sl + n, total, g0, g1);
    else if (n < total + CO) s = slab_sum(bs + (n - total), CO, g0, g1);
    part[grp][nl] = s;
    __syncthreads();
    if (grp == 0 && n < total + CO) {
        float v = 0.f;
#pragma unroll
        for (int i = 0; i < 16; ++i) v += part[i][nl];
        if (n < total) {
            int co = n / 288, rem = n % 288, tap = rem / 32, ci = rem % 32;
            dw[((long)(cob * CO + co) * cin_total + cib * 32 + ci) * 9 + tap] = v;
        } else if (cib == 0) {
            db[cob * CO + (n - total)] = v;
        }
    }
}

// ------------------------------------------------------------------------------------------------
// weight gradient, CIN = 3, COUT = 32: one 32 x 32 MFMA tile (27 of 32 columns used), K = pixels.
// ------------------------------------------------------------------------------------------------
template <int W>
struct Wg3Cfg {
    static constexpr int COUT = 32, CIN = 3;
    static constexpr int NPIX = 2 * W;
    static constexpr int LDP = NPIX + 1;
    static constexpr int LDW = W + 8 + 3;            // 139 for W=128: = 11 mod 32 (taps spread over banks)
    static constexpr int PLANE = 4 * LDW + 5;
    static constexpr int DYF = COUT * LDP;
    static constexpr int XF = CIN * PLANE + 8;
    static constexpr int BUF = DYF + XF;
    static constexpr size_t LDS_BYTES = (size_t)2 * BUF * sizeof(float);
};

template <int W>
__global__ __launch_bounds__(512) void conv_wgrad3_kernel(WgradParams p) {
    using C = Wg3Cfg<W>;
    constexpr int COUT = 32, CIN = 3, LDP = C::LDP, LDW = C::LDW, PLANE = C::PLANE;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int H = p.H, Hp = H / 2, Wp = W / 2;
    const int strips_per_img = H / 2;
    const int nstrips = p.B * strips_per_img;
    const int cob = blockIdx.x / p.groups, grp = blockIdx.x % p.groups;   // 32-output-channel block, group within it
    const int COUT_T = p.cout_total;
    for (int i = t; i < 2 * C::BUF; i += 512) smem[i] = 0.f;
    __syncthreads();

    constexpr int DY_ITEMS = COUT * (Wp / 4);
    constexpr int DY_NIT = (DY_ITEMS + 511) / 512;
    constexpr int X_ITEMS = CIN * 4 * (W / 4);
    constexpr int X_NIT = (X_ITEMS + 511) / 512;
    float4 gq[DY_NIT]; uint32_t mq[DY_NIT]; float4 xq[X_NIT];
    float bsum[DY_NIT];      // bias-gradient partial of this thread's fixed channel
#pragma unroll
    for (int i = 0; i < DY_NIT; ++i) bsum[i] = 0.f;
    auto load_stage = [&](int strip) __attribute__((always_inline)) {
        const int b = strip / strips_per_img, ph = strip % strips_per_img, h0 = ph * 2;
        // unconditional loads from clamped addresses (a load under a per-item `if` makes hipcc wait vmcnt(0) at the
        // join and exposes the HBM latency every strip); out-of-range items are zeroed with selects afterwards
#pragma unroll
        for (int i = 0; i < DY_NIT; ++i) {
            int idx = min(t + i * 512, DY_ITEMS - 1);
            int q = idx % (Wp / 4), co = idx / (Wp / 4);
            long off = (((long)b * COUT_T + cob * COUT + co) * Hp + ph) * Wp + q * 4;
            gq[i] = *reinterpret_cast<const float4*>(p.gy + off);
            mq[i] = *reinterpret_cast<const uint32_t*>(p.mask + off);
        }
#pragma unroll
        for (int i = 0; i < X_NIT; ++i) {
            int idx = min(t + i * 512, X_ITEMS - 1);
            int q = idx % (W / 4), row = (idx / (W / 4)) % 4, ci = idx / (W / 4 * 4);
            int hh = h0 - 1 + row;
            const bool ok = hh >= 0 && hh < H;
            float4 v = *reinterpret_cast<const float4*>(p.x + (((long)b * CIN + ci) * H + min(max(hh, 0), H - 1)) * W + q * 4);
            xq[i].x = ok ? v.x : 0.f; xq[i].y = ok ? v.y : 0.f; xq[i].z = ok ? v.z : 0.f; xq[i].w = ok ? v.w : 0.f;
        }
    };
    auto store_stage = [&](int buf) __attribute__((always_inline)) {
        float* dys = smem + buf * C::BUF;
        float* xs = dys + C::DYF;
#pragma unroll
        for (int i = 0; i < DY_NIT; ++i) {
            int idx = t + i * 512;
            if (idx >= DY_ITEMS) continue;
            int q = idx % (Wp / 4), co = idx / (Wp / 4);
            float* d = dys + co * LDP + q * 8;
            float g[4] = {gq[i].x, gq[i].y, gq[i].z, gq[i].w};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                uint32_t m = (mq[i] >> (8 * e)) & 0xff;
                bsum[i] += m < 4 ? g[e] : 0.f;
                d[2 * e] = m == 0 ? g[e] : 0.f;
                d[2 * e + 1] = m == 1 ? g[e] : 0.f;
                d[W + 2 * e] = m == 2 ? g[e] : 0.f;
                d[W + 2 * e + 1] = m == 3 ? g[e] : 0.f;
            }
        }
#pragma unroll
        for (int i = 0; i < X_NIT; ++i) {
            int idx = t + i * 512;
            if (idx >= X_ITEMS) continue;
            int q = idx % (W / 4), row = (idx / (W / 4)) % 4, ci = idx / (W / 4 * 4);
            float* d = xs + ci * PLANE + row * LDW + PADL + q * 4;
            d[0] = xq[i].x; d[1] = xq[i].y; d[2] = xq[i].z; d[3] = xq[i].w;
        }
    };

    constexpr int PIX_PER_W = C::NPIX / 8;             // pixels per wave per strip
    const int pix0 = wave * PIX_PER_W;
    const int prow = pix0 / W, pcol = pix0 % W;
    const int j = lane & 31, k2 = lane >> 5;
    // column j <-> (ci, kh, kw) = (j / 9, (j % 9) / 3, j % 3) for j < 27
    const int jj = j < 27 ? j : 0;
    const int boff = (jj / 9) * PLANE + ((jj % 9) / 3) * LDW + (jj % 3);
    const int abase = j * LDP + pix0 + k2;
    const int bbase = boff + prow * LDW + pcol + k2 + PADL - 1;
    const float bsel = j < 27 ? 1.f : 0.f;

    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;

    int strip = xcd_adjacent(grp, p.groups);       // groups % 8 == 0 keeps id % 8 == grp % 8 for every (channel block) pair; else identity
    if (strip < nstrips) { load_stage(strip); store_stage(0); }
    __syncthreads();
    int buf = 0;
    for (; strip < nstrips; strip += p.groups) {
        const int nstrip = strip + p.groups;
        if (nstrip < nstrips) load_stage(nstrip);
        const float* dys = smem + buf * C::BUF + abase;
        const float* xs = smem + buf * C::BUF + C::DYF + bbase;
#pragma unroll
        for (int pp = 0; pp < PIX_PER_W; pp += 2) acc = mfma32(dys[pp], xs[pp] * bsel, acc);
        if (nstrip < nstrips) store_stage(buf ^ 1);
        __syncthreads();
        buf ^= 1;
    }
    float* red = smem;
    for (int g = 1; g < 8; ++g) {
        if (wave == g) {
#pragma unroll
            for (int r = 0; r < 16; ++r) red[r * 64 + lane] = acc[r];
        }
        __syncthreads();
        if (wave == 0) {
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[r] += red[r * 64 + lane];
        }
        __syncthreads();
    }
    // bias-gradient partials: the Wp/4 consecutive lanes of one channel reduce by shuffles
#pragma unroll
    for (int i = 0; i < DY_NIT; ++i) {
        float v = bsum[i];
#pragma unroll
        for (int o = 1; o < Wp / 4; o <<= 1) v += __shfl_xor(v, o);
        int idx = t + i * 512;
        if (idx < DY_ITEMS && idx % (Wp / 4) == 0) p.bslab[(long)blockIdx.x * COUT + idx / (Wp / 4)] = v;
    }
    if (wave == 0) {
        float* s = p.slab + (long)blockIdx.x * 1024;
#pragma unroll
        for (int r = 0; r < 16; ++r) s[mfma_row(r, lane) * 32 + j] = acc[r];
    }
}

// dW[cob*32+co][27] = sum_g slab[cob][g][co][j], j = ci*9 + tap; db[cob*32+co] = sum_g bslab[cob][g][co].
// grid (33, cout/32): a block owns 32 outputs; its 8 thread groups each sum a fixed eighth of the slabs.
__global__ __launch_bounds__(1024) void conv_wgrad3_reduce_kernel(const float* slab, const float* bslab, float* dw,
                                                                 float* db, int groups) {
    __shared__ float part[32][32];
    const int cob = blockIdx.y;
    const float* sl = slab + (long)cob * groups * 1024;
    const float* bs = bslab + (long)cob * groups * 32;
    const int nl = threadIdx.x & 31, grp = threadIdx.x >> 5;
    const int n = blockIdx.x * 32 + nl;          // 0..1023 weights (32 blocks), 1024..1055 biases (block 32)
    const int per = (groups + 31) / 32, g0 = min(groups, grp * per), g1 = min(groups, g0 + per);
    float s = 0.f;
    if (n < 1024) s = slab_sum(sl + n, 1024, g0, g1);
    else s = slab_sum(bs + (n - 1024), 32, g0, g1);
    part[grp][nl] = s;
    __syncthreads();
    if (grp == 0) {
        float v = 0.f;
#pragma unroll
        for (int i = 0; i < 32; ++i) v += part[i][nl];
        if (n < 1024) { if ((n & 31) < 27) dw[(cob * 32 + (n >> 5)) * 27 + (n & 31)] = v; }
        else db[cob * 32 + (n - 1024)] = v;
    }
}

template <int CIN, int COUT, int W, int MODE>
int launch_conv(const ConvParams& p, hipStream_t st) {
    using C = ConvCfg<CIN, COUT, W, MODE>;
    // 4-wave work-groups, 2-4 per CU: the co-resident groups hit their per-chunk barriers at different times, so a
    // SIMD's MFMA pipe keeps being fed by the other group's wave (one 8-wave group per CU measured 79 % MFMA busy).
    // With reserved CUs (two-branch overlap experiments): one work-group per CU, LDS request raised to >= 120 KB.
    const bool part = g_bbbp_reserved_cus > 0;
    size_t lds = C::LDS_BYTES;
    if (part && lds < BBBP_CONV_MIN_LDS) lds = BBBP_CONV_MIN_LDS;
    int nstrips = p.B * (p.H / C::TH);
    int per_cu = (int)((160 * 1024) / lds);
    if (per_cu > 2) per_cu = 2;      // measured: more than 2 groups per CU buys nothing and crowds out the side-stream kernels
    if (per_cu < 1) per_cu = 1;
    static const int cap = bbbp_env_int("BBBP_CONV_PER_CU", 0);
    if (cap > 0 && per_cu > cap) per_cu = cap;
    int cus = bbbp_num_cus() - (part ? g_bbbp_reserved_cus : 0);
    if (cus < 1) cus = 1;
    int grid = cus * per_cu;
    if (grid > nstrips) grid = nstrips;
    return launch_lds(conv3x3_kernel<CIN, COUT, W, MODE>, grid, C::NT, lds, st, p);
}

// shapes on the reference's paths: the flagship CNN (3->32 @128, 32->64 @64; ...20250113.py:84-90) and the wide/deep
// variant (3->64 @128, 64->128 @64, 128->256 @32; ..._opt_20250107_network.py:129-138)
inline bool supported(int cin, int cout, int h, int w) {
    if (h != w) return false;
    return (cin == 3 && cout == 32 && w == 128) || (cin == 32 && cout == 64 && w == 64) || (cin == 3 && cout == 64 && w == 128) ||
           (cin == 64 && cout == 128 && w == 64) || (cin == 128 && cout == 256 && w == 32);
}

// BBBP_CONV_WINOGRAD (bbbp_set_conv_winograd): the ConvMaskBit set (common.h).  Default since round 2: conv2's three ops as split-bf16 (28; the
// weight gradient alone 0.63 -> 0.42 ms, and beside it the encoder's backward chain runs 1.93 -> 1.45 ms: 4 waves x 180 registers instead of
// conv_wgrad32's 8 x 224) -- alone as fast as the Winograd form (0.42 / 0.41 vs 0.42 / 0.44 ms at B = 512), and in the training step 0.47 / 0.42
// vs 0.57 / 0.61 ms: 66 KB of LDS and 160 registers per wave leave room for the other branch's kernels on every CU (the Winograd work-groups
// take whole CUs and give 64 of them up), and a bf16 MFMA holds the vector issue for 8 of its 32 cycles where the f32 MFMA blocks it for all 64.
// Round 3: + conv1's split-bf16 forms and conv2's weight gradient on the structured-sparse MFMA (0.54 -> 0.33 ms in the step).
Knob g_winograd{"BBBP_CONV_WINOGRAD", 252, [](int v) { return v & CONV_MASK_ALL; }};
// the calling thread's two settable form choices (bbbp_set_conv2_fwd_pipe, bbbp_set_conv_wgrad_beside_encoder): read by the C entry points only
thread_local int g_bbbp_conv2_fwd_pipe = 0;
thread_local int g_bbbp_conv_wgrad_beside_encoder = 0;

// The environment's say in the choice below, read once per process
struct ConvKnobs {
    int c2_pipe;               // BBBP_C2_PIPE: set (any integer), it wins over every caller's ConvPrefs::conv2_fwd_pipe; INT_MIN = unset
    int c2_dgrad_pipe;         // BBBP_C2_DGRAD_PIPE: the pipelined kernel for the data gradient of the 64 x 64-map stages (default off)
    int b3_probe;              // BBBP_B3_PROBE: the phase-stamping build of the flagship split-bf16 kernel (bbbp_conv_b3_phases); never pipelined
    int b3_per_cu;             // BBBP_B3_PER_CU: work-groups per CU of the split-bf16 conv2-family kernels, 1 or 2 (default 2)
    int wgrad_sparse_waves;    // BBBP_C2_WGRAD_SPARSE_WAVES: 8 or 4 forces that structured-sparse form (0: by mask and preference)
    int c1_pipe;               // BBBP_C1_PIPE: round 4's software-pipelined conv1 forward (0: round 3's phase-by-phase kernel)
    int c1_per_cu;             // BBBP_C1_PER_CU: its work-groups per CU, 1..4 (default 2), where the caller has no preference
};
const ConvKnobs& conv_knobs() {
    static const ConvKnobs k{bbbp_env_int("BBBP_C2_PIPE", INT_MIN), bbbp_env_int("BBBP_C2_DGRAD_PIPE", 0), bbbp_env_int("BBBP_B3_PROBE", 0),
                             clampi(bbbp_env_int("BBBP_B3_PER_CU", 2), 1, 2), bbbp_env_int("BBBP_C2_WGRAD_SPARSE_WAVES", 0),
                             bbbp_env_int("BBBP_C1_PIPE", 1), clampi(bbbp_env_int("BBBP_C1_PER_CU", 2), 1, 4)};
    return k;
}

enum class ConvOp { Fwd, Dgrad, Wgrad };
enum class ConvClock { Keep, F32, Winograd, SplitBf16 };      // whose stamps bbbp_conv_last_clock reads after the call (Keep: the op leaves none)
struct ConvChoice {
    ConvForm form = ConvForm::F32Direct;
    size_t workspace = 0;      // bytes the call needs: prepared filters (forward, data gradient) or partial slabs (weight gradient)
    ConvClock clock = ConvClock::F32;
    int per_cu = 0;            // split-bf16 forward / data gradient: work-groups per CU
    bool probe = false;        // ConvKnobs::b3_probe
};
ConvClock g_last_clock = ConvClock::F32;

// The one place a conv call's kernel form is chosen (shapes: `supported` above; hw = map height = width).
ConvChoice conv_choice(ConvOp op, int cin, int cout, int hw, int mask, const ConvPrefs& prefs, const ConvKnobs& kn) {
    ConvChoice c;
    const bool b3_stage = bbbp_b3_conv_supported(cin, cout, hw), conv2 = cin == 32 && cout == 64, conv1 = cin == 3 && cout == 32 && hw == 128;
    auto at_least = [&](size_t bytes) { if (c.workspace < bytes) c.workspace = bytes; };
    if (op == ConvOp::Wgrad) {
        // slabs of any grid: pairs * groups <= 2 * 256 work-groups (the entry point checks its own grid's share)
        c.workspace = (size_t)2 * 256 * (cin == 3 ? 1024 + 32 : (size_t)64 * 288 + 64) * sizeof(float);
        c.clock = ConvClock::Keep;
        const bool sparse = (mask & CONV_B3_WGRAD_SPARSE) != 0;
        if (conv1 && (mask & CONV_B3_C1_WGRAD)) c.form = ConvForm::Conv1SplitBf16;
        // split-bf16 weight gradient, (32 ci, 64 co) block pairs: dense or sparse on 64 x 64 maps (the flagship's second stage, one pair; the
        // wide / deep variant's 64 -> 128 stage, four pairs), sparse only on the variant's 32 x 32 third stage (16 pairs; a stage = two pooled rows)
        else if (b3_stage && (mask & CONV_B3_WGRAD) && (sparse || hw == 64)) {
            // the sparse form has an 8-wave kernel (fastest alone: two waves of 256 registers per SIMD) and a 4-wave one that leaves ~200
            // registers per lane slot to the fingerprint branch's kernels: the engine asks for that while an encoder chain runs beside
            const int waves = kn.wgrad_sparse_waves ? kn.wgrad_sparse_waves : (((mask & CONV_B3_WGRAD_SPARSE4) || prefs.wgrad_beside_encoder) ? 4 : 8);
            c.form = !sparse ? ConvForm::WgradDense : waves == 8 ? ConvForm::WgradSparse8 : ConvForm::WgradSparse4;
        }
        return c;
    }
    const bool fwd = op == ConvOp::Fwd;
    c.workspace = (size_t)9 * (fwd && cin < 8 ? 4 : cin) * cout * sizeof(float);      // the f32 kernels' re-laid filters; every form's floor
    if (b3_stage && (mask & (fwd ? CONV_B3_FWD : CONV_B3_DGRAD))) {
        // 64 x 64 maps have a software-pipelined one-work-group-per-CU kernel: 3 % slower alone, but it leaves an encoder chain beside it
        // three quarters of every SIMD (step 2.8 % faster), so the engine asks for it in training plans with an encoder
        const int pipe = !fwd ? kn.c2_dgrad_pipe : kn.c2_pipe != INT_MIN ? kn.c2_pipe : prefs.conv2_fwd_pipe;
        c.form = (hw == 64 && pipe && !kn.b3_probe) ? ConvForm::SplitBf16Pipe : ConvForm::SplitBf16;
        c.per_cu = kn.b3_per_cu; c.probe = kn.b3_probe != 0;
        c.clock = ConvClock::SplitBf16;
        at_least(bbbp_b3_workspace_bytes(cin, cout));
    } else if (conv2 && (mask & (fwd ? CONV_WINO_FWD : CONV_WINO_DGRAD))) {
        c.form = ConvForm::Winograd;
        c.clock = ConvClock::Winograd;
        at_least((size_t)16 * 32 * 64 * sizeof(float));
    } else if (fwd && conv1 && (mask & CONV_B3_C1_FWD) && !prefs.conv1_fwd_f32) {
        // Faster alone than the f32 kernel (0.19 vs 0.26 ms at B = 512) but it holds 2 x 248 registers per lane slot on every SIMD, and a
        // training step's forward is bound by the encoder's latency chain, which then finds no wave slots (measured: conv1 0.31 -> 0.20 ms
        // in-step, encoder forward 1.21 -> 1.33, step 2.61 -> 2.70): the engine sets conv1_fwd_f32 there, or asks the pipelined form -- which
        // keeps the matrix pipe busy with ONE wave per SIMD -- for one work-group per CU (half the register file and 100 KB of LDS stay free)
        c.form = kn.c1_pipe ? ConvForm::Conv1SplitBf16Pipe : ConvForm::Conv1SplitBf16;
        c.per_cu = prefs.conv1_fwd_per_cu > 0 ? prefs.conv1_fwd_per_cu : kn.c1_per_cu;
        at_least(bbbp_b3_conv1_fwd_workspace_bytes());      // the kernel stamps no clock of its own: bbbp_conv_last_clock keeps reading the f32 pair
    }
    return c;
}
ConvChoice conv_choice(ConvOp op, int cin, int cout, int hw, const ConvPrefs& prefs) { return conv_choice(op, cin, cout, hw, g_winograd.get(), prefs, conv_knobs()); }

}  // namespace

extern "C" int bbbp_set_conv_winograd(int mask) {
    BBBP_CHECK_ARG(mask >= 0 && mask <= CONV_MASK_ALL, "set_conv_winograd: mask %d (bits 0/1 Winograd forward / data gradient, bits 2/3/4 split-bf16 forward / data gradient / weight gradient of conv2, bits 5/6 split-bf16 weight gradient / forward of conv1, bit 7 conv2's split-bf16 weight gradient on the structured-sparse MFMA, bit 8 its 4-wave form)", mask);
    g_winograd.set(mask);
    return BBBP_OK;
}

extern "C" int bbbp_get_conv_winograd(void) { return g_winograd.get(); }
extern "C" int bbbp_conv_winograd_phases(unsigned long long* phases4) {
    BBBP_CHECK_ARG(phases4, "conv_winograd_phases: null pointer");
    return bbbp_wino_last_phases(phases4);
}

extern "C" int bbbp_conv_last_clock(unsigned long long* shader_cycles, unsigned long long* ticks_100mhz) {
    BBBP_CHECK_ARG(shader_cycles && ticks_100mhz, "conv_last_clock: null pointer");
    if (g_last_clock == ConvClock::SplitBf16) return bbbp_b3_last_clock(shader_cycles, ticks_100mhz);
    if (g_last_clock == ConvClock::Winograd) return bbbp_wino_last_clock(shader_cycles, ticks_100mhz);
    unsigned long long h[2] = {0, 0};
    BBBP_CHECK_HIP(hipMemcpyFromSymbol(h, HIP_SYMBOL(g_conv_clock), sizeof(h)));
    *shader_cycles = h[0]; *ticks_100mhz = h[1];
    return BBBP_OK;
}

// workspace for any of the three ops on this stage, whatever form the mask, the caller or the knobs select
extern "C" size_t bbbp_conv3x3_workspace_bytes(int B, int cin, int cout, int H, int W) {
    (void)B; (void)W;
    auto need = [&](ConvOp op) { return conv_choice(op, cin, cout, H, ConvPrefs{}).workspace; };
    return align_up(std::max({need(ConvOp::Fwd), need(ConvOp::Dgrad), need(ConvOp::Wgrad)}), 256);
}

// The calling thread's two preferences (include/bbbp_hip.h); each returns the previous setting.  BBBP_C2_PIPE=0 / 1 overrides every caller.
extern "C" int bbbp_set_conv_wgrad_beside_encoder(int on) {
    const int prev = g_bbbp_conv_wgrad_beside_encoder;
    g_bbbp_conv_wgrad_beside_encoder = on ? 1 : 0;
    return prev;
}
extern "C" int bbbp_set_conv2_fwd_pipe(int on) {
    const int prev = g_bbbp_conv2_fwd_pipe;
    g_bbbp_conv2_fwd_pipe = on ? 1 : 0;
    return prev;
}

// The form the matching C entry point would run right now (include/bbbp_hip.h): the same conv_choice under the same mask, the calling
// thread's two preferences and the knobs.  Host side only.
extern "C" int bbbp_conv_kernel_form(int op, int cin, int cout, int hw) {
    if (op < 0 || op > 2 || !supported(cin, cout, hw, hw) || (op == 1 && cin == 3)) return -1;
    ConvPrefs prefs;
    prefs.conv2_fwd_pipe = g_bbbp_conv2_fwd_pipe;
    prefs.wgrad_beside_encoder = g_bbbp_conv_wgrad_beside_encoder;
    const ConvOp ops[3] = {ConvOp::Fwd, ConvOp::Dgrad, ConvOp::Wgrad};
    return (int)conv_choice(ops[op], cin, cout, hw, prefs).form;
}

extern "C" int bbbp_conv3x3_relu_pool_fwd(void* stream, const float* x, const float* w, const float* bias,
                                          float* y, uint8_t* mask, int B, int cin, int cout, int H, int W,
                                          void* workspace, size_t workspace_bytes) {
    ConvPrefs prefs;
    prefs.conv2_fwd_pipe = g_bbbp_conv2_fwd_pipe;
    return conv3x3_relu_pool_fwd(static_cast<hipStream_t>(stream), x, w, bias, y, mask, B, cin, cout, H, W, workspace, workspace_bytes, prefs);
}

int conv3x3_relu_pool_fwd(hipStream_t st, const float* x, const float* w, const float* bias, float* y, uint8_t* mask, int B, int cin, int cout,
                          int H, int W, void* workspace, size_t workspace_bytes, const ConvPrefs& prefs) {
    BBBP_CHECK_ARG(supported(cin, cout, H, W), "conv fwd: unsupported shape cin=%d cout=%d H=%d W=%d", cin, cout, H, W);
    BBBP_CHECK_ARG(x && w && bias && y && workspace, "conv fwd: null pointer");      // mask may be null: forward-only call, no decisions kept
    if (B == 0) return BBBP_OK;
    const ConvChoice c = conv_choice(ConvOp::Fwd, cin, cout, H, prefs);
    BBBP_CHECK_ARG(workspace_bytes >= c.workspace, "conv fwd: workspace %zu < %zu", workspace_bytes, c.workspace);
    float* wt = static_cast<float*>(workspace);
    g_last_clock = c.clock;
    if (c.form == ConvForm::SplitBf16 || c.form == ConvForm::SplitBf16Pipe)
        return bbbp_b3_conv_fwd(st, x, w, bias, y, mask, B, cin, cout, workspace, c.form, c.per_cu, c.probe);
    if (c.form == ConvForm::Winograd) return bbbp_wino_conv2_fwd(st, x, w, bias, y, mask, B, wt);
    if (c.form != ConvForm::F32Direct) return bbbp_b3_conv1_fwd(st, x, w, bias, y, mask, B, workspace, c.form, c.per_cu);
    const int cinp = cin < 8 ? 4 : cin, total = 9 * cinp * cout;
    hipLaunchKernelGGL(conv_prep_weights_kernel, dim3(cdiv(total, 256)), dim3(256), 0, st, w, wt, cin, cout, cinp, MODE_FWD);
    BBBP_CHECK_LAUNCH();
    ConvParams p{x, nullptr, wt, bias, y, mask, B, H, cout};
    if (cin == 3 && cout == 32) return launch_conv<3, 32, 128, MODE_FWD>(p, st);
    if (cin == 3 && cout == 64) return launch_conv<3, 64, 128, MODE_FWD>(p, st);
    if (cin == 32) return launch_conv<32, 64, 64, MODE_FWD>(p, st);
    if (cin == 64) return launch_conv<64, 64, 64, MODE_FWD>(p, st);
    return launch_conv<128, 64, 32, MODE_FWD>(p, st);
}

// dx[B][cin][H][W] from the pooled output gradient gy[B][cout][H/2][W/2] and the forward mask
extern "C" int bbbp_conv3x3_relu_pool_bwd_data(void* stream, const float* gy, const uint8_t* mask, const float* w,
                                               float* dx, int B, int cin, int cout, int H, int W,
                                               void* workspace, size_t workspace_bytes) {
    BBBP_CHECK_ARG(supported(cin, cout, H, W) && cin != 3,
                   "conv bwd_data: unsupported shape cin=%d cout=%d H=%d W=%d", cin, cout, H, W);
    BBBP_CHECK_ARG(gy && mask && w && dx && workspace, "conv bwd_data: null pointer");
    if (B == 0) return BBBP_OK;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const ConvChoice c = conv_choice(ConvOp::Dgrad, cin, cout, H, ConvPrefs{});
    BBBP_CHECK_ARG(workspace_bytes >= c.workspace, "conv bwd_data: workspace %zu < %zu", workspace_bytes, c.workspace);
    float* wt = static_cast<float*>(workspace);
    g_last_clock = c.clock;
    if (c.form == ConvForm::SplitBf16 || c.form == ConvForm::SplitBf16Pipe)
        return bbbp_b3_conv_dgrad(st, gy, mask, w, dx, B, cin, cout, workspace, c.form, c.per_cu, c.probe);
    if (c.form == ConvForm::Winograd) return bbbp_wino_conv2_dgrad(st, gy, mask, w, dx, B, wt);
    int total = 9 * cout * cin;
    hipLaunchKernelGGL(conv_prep_weights_kernel, dim3(cdiv(total, 256)), dim3(256), 0, st, w, wt, cin, cout, 0, MODE_DGRAD);
    BBBP_CHECK_LAUNCH();
    // the data-gradient conv reads cout channels and writes cin channels
    ConvParams p{gy, mask, wt, nullptr, dx, nullptr, B, H, cin};
    if (cin == 32) return launch_conv<64, 32, 64, MODE_DGRAD>(p, st);
    if (cin == 64) return launch_conv<128, 64, 64, MODE_DGRAD>(p, st);
    return launch_conv<256, 64, 32, MODE_DGRAD>(p, st);
}

template <int W, int CIN_TOTAL, int COUT_TOTAL>
static int launch_wgrad32(WgradParams p, int grid, hipStream_t st) {
    return launch_lds(conv_wgrad32_kernel<64, W, CIN_TOTAL, COUT_TOTAL>, grid, 512, WgCfg<64, W>::LDS_BYTES, st, p);
}

// dw[cout][cin][3][3], db[cout] from the layer input x, the pooled output gradient and the mask
extern "C" int bbbp_conv3x3_relu_pool_bwd_weight(void* stream, const float* x, const float* gy, const uint8_t* mask,
                                                 float* dw, float* db, int B, int cin, int cout, int H, int W,
                                                 void* workspace, size_t workspace_bytes) {
    ConvPrefs prefs;
    prefs.wgrad_beside_encoder = g_bbbp_conv_wgrad_beside_encoder;
    return conv3x3_relu_pool_bwd_weight(static_cast<hipStream_t>(stream), x, gy, mask, dw, db, B, cin, cout, H, W, workspace, workspace_bytes, prefs);
}

int conv3x3_relu_pool_bwd_weight(hipStream_t st, const float* x, const float* gy, const uint8_t* mask, float* dw, float* db, int B, int cin,
                                 int cout, int H, int W, void* workspace, size_t workspace_bytes, const ConvPrefs& prefs) {
    BBBP_CHECK_ARG(supported(cin, cout, H, W), "conv bwd_weight: unsupported shape cin=%d cout=%d H=%d W=%d", cin, cout, H, W);
    BBBP_CHECK_ARG(x && gy && mask && dw && db && workspace, "conv bwd_weight: null pointer");
    if (B == 0) {
        BBBP_CHECK_HIP(hipMemsetAsync(dw, 0, (size_t)cout * cin * 9 * sizeof(float), st));
        BBBP_CHECK_HIP(hipMemsetAsync(db, 0, (size_t)cout * sizeof(float), st));
        return BBBP_OK;
    }
    const ConvChoice c = conv_choice(ConvOp::Wgrad, cin, cout, H, prefs);
    int nstrips = B * (H / 2);
    const bool part = g_bbbp_reserved_cus > 0;
    const int ncu = bbbp_num_cus(), cus = ncu - (part ? g_bbbp_reserved_cus : 0) > 0 ? ncu - (part ? g_bbbp_reserved_cus : 0) : 1;
    float* slab = static_cast<float*>(workspace);
    WgradParams p{x, gy, mask, slab, nullptr, B, H, cin, cout, 1};
    if (cin == 3) {
        using C = Wg3Cfg<128>;
        const int ncob = cout / 32;
        size_t lds3 = C::LDS_BYTES;
        if (part) lds3 = BBBP_CONV_MIN_LDS;          // one per CU on the unreserved CUs
        const int groups = clampi((part ? cus : ncu * 2) / ncob, 1, nstrips);
        const int grid = groups * ncob;
        BBBP_CHECK_ARG(workspace_bytes >= (size_t)grid * (1024 + 32) * sizeof(float), "conv bwd_weight: workspace too small");
        p.groups = groups;
        p.bslab = slab + (size_t)grid * 1024;
        const int rc = c.form == ConvForm::Conv1SplitBf16 ? bbbp_b3_conv1_wgrad(st, x, gy, mask, slab, p.bslab, B, grid)
                                                          : launch_lds(conv_wgrad3_kernel<128>, grid, 512, lds3, st, p);
        if (rc) return rc;
        hipLaunchKernelGGL(conv_wgrad3_reduce_kernel, dim3(33, ncob), dim3(1024), 0, st, slab, p.bslab, dw, db, groups);
        BBBP_CHECK_LAUNCH();
    } else {
        const int pairs = (cin / 32) * (cout / 64);
        const int groups = clampi(cus / pairs, 1, nstrips);
        const int grid = groups * pairs;
        BBBP_CHECK_ARG(workspace_bytes >= (size_t)grid * (64 * 288 + 64) * sizeof(float), "conv bwd_weight: workspace too small");
        p.groups = groups;
        p.bslab = slab + (size_t)grid * 64 * 288;
        int rc;
        if (c.form != ConvForm::F32Direct) rc = bbbp_b3_conv2_wgrad(st, x, gy, mask, slab, p.bslab, B, grid, c.form, cin, cout, groups, W);
        else rc = cin == 32 ? launch_wgrad32<64, 32, 64>(p, grid, st)
               : cin == 64 ? launch_wgrad32<64, 64, 128>(p, grid, st) : launch_wgrad32<32, 128, 256>(p, grid, st);
        if (rc) return rc;
        hipLaunchKernelGGL(conv_wgrad32_reduce_kernel, dim3(cdiv(64 * 289, 64), pairs), dim3(1024), 0, st, slab, p.bslab, dw, db,
                           groups, cin, cout);
        BBBP_CHECK_LAUNCH();
    }
    return BBBP_OK;
}
