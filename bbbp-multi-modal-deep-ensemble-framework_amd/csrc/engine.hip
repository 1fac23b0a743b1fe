// Whole-model orchestration of MixedInputModel forward / backward on one MI355X: the host-side
// schedule that strings the gfx950 kernels (gemm.hip, conv.hip, rowops.hip) together on one HIP stream
// with a single caller-provided workspace (no allocation, no synchronisation: graph-capturable).
//
// Reference: MixedInputModel.forward, Models/multi_input_data_regression_opt_transformer_cnn_20250113.py:109-119
// (R below) and its autograd under loss.backward() (R:190).  The encoder is called with a [B,1,F]
// tensor and batch_first=False (R:110-111), so self-attention runs ACROSS the mini-batch: S = B, N = 1.
#include "common.h"
#include "attention_b3.h"
#include "encoder_sliced.h"
#include "head_sync.h"
#include <optional>
#include "bbbp_hip.h"
#include <mutex>
#include <stdlib.h>

namespace {

constexpr int IMG = 128, C1 = 32, C2 = 64, FC = 128, NHEADS_FUSION = 4, FUS_HID = 128;
constexpr int H1 = 256, H2 = 128, H3 = 64;
constexpr int COMB = 2 * FC;          // 256
constexpr int IMG_FLAT = C2 * (IMG / 4) * (IMG / 4);   // 65536

// parameter indices in named_parameters() order
enum { L_INW = 0, L_INB, L_OUTW, L_OUTB, L_W1, L_B1, L_W2, L_B2, L_N1W, L_N1B, L_N2W, L_N2B, L_COUNT };
struct PIdx {
    int L, NF;             // NF: parameter tensors of the fusion block (16 for MultiHeadAttentionFusion, 0 for torch.cat)
    PIdx(int layers, int fusion) : L(layers), NF(fusion == 0 ? 4 * NHEADS_FUSION : 0) {}
    explicit PIdx(const bbbp_mixed_desc* d) : PIdx(d->num_layers, d->fusion) {}
    int layer(int l, int k) const { return l * L_COUNT + k; }
    int base() const { return L * L_COUNT; }
    int fpfc_w() const { return base() + 0; }
    int fpfc_b() const { return base() + 1; }
    int c1_w() const { return base() + 2; }
    int c1_b() const { return base() + 3; }
    int c2_w() const { return base() + 4; }
    int c2_b() const { return base() + 5; }
    int ifc_w() const { return base() + 6; }
    int ifc_b() const { return base() + 7; }
    int fus(int h, int k) const { return base() + 8 + h * 4 + k; }     // k: 0 W1, 1 b1, 2 w2, 3 b2
    int fc0_w() const { return base() + 8 + NF; }
    int fc0_b() const { return base() + 9 + NF; }
    int bn_w() const { return base() + 10 + NF; }
    int bn_b() const { return base() + 11 + NF; }
    int fc3_w() const { return base() + 12 + NF; }
    int fc3_b() const { return base() + 13 + NF; }
    int fc5_w() const { return base() + 14 + NF; }
    int fc5_b() const { return base() + 15 + NF; }
    int fc7_w() const { return base() + 16 + NF; }
    int fc7_b() const { return base() + 17 + NF; }
    int count() const { return base() + 18 + NF; }
};

struct Bump {
    size_t off = 0;
    size_t take(size_t bytes) { size_t o = off; off = align_up(off + bytes, 256); return o; }
    size_t f(size_t n) { return take(n * sizeof(float)); }
};

struct LayerOff { size_t qkv, prob, pd, ctx, z1, y1, hff, z2, y2, mean1, rstd1, mean2, rstd2, lse, keep, kvg; };      // keep: 0 = none; kvg: exact-global-batch mode only
// per-layer gradient buffers: weight-gradient kernels read them on a third stream while the dependency
// chain moves on to the next layer, so they must not be recycled within one backward pass
struct LayerGrad { size_t dyout, dz2, dz2d, dhff, dy1, dz1, dz1d, dqkv; };

struct Plan {
    int B, F, NH, D, L, DFF;
    bool drop, concat, inference;
    bool flash;            // many heads of head_dim 8 / 16: fused attention (attention.hip), no [NH,B,B] probability tensors
    size_t sl_sync, sl_part;   // sliced persistent forward: barrier counters, linear2 partials (allocated whenever the shape is supported)
    size_t sl_kvpart;          // sliced persistent backward: every row block's share of dK | dV (training plans only)
    // exact-global-batch mode (bbbp_mixed_desc.collective): B is this rank's shard, keys / values / BatchNorm statistics span Bg = world * B rows
    bool exact; int world, rank; size_t Bg;
    size_t dkvg, dkvl;         // this rank's queries' share of dK | dV for all Bg keys; the reduce-scattered rows of this rank
    bool attn_b3;          // forward-only plan, wide head, >= 1024 rows: split-bf16 attention (attention_b3.hip)
    // one-head layers on the launch-per-op schedule: out_proj folded into the value projection (fold.hip); per layer the folded in_proj
    // weight / bias, [Wv | bv]^T, and (training plans) the folded gradient dW' | db'
    bool fold; size_t fwf[32], fbf[32], fwvt[32], ftdw[32], ftdb[32];
    size_t attn_part, attn_part_bytes;
    LayerOff layer[32];
    LayerGrad lgrad[32];
    size_t scratch3, scratch3_bytes;
    size_t seed_slot;      // the call's dropout seed, in device memory (common.h: effective_seed)
    size_t pool1, mask1, pool2, mask2;
    size_t combined, hid, attn, fused, h, hb, bn_mean, bn_rstd, h2, h3, head_partial;
    // temporaries
    size_t scratch, scratch_bytes, scratch2, scratch2_bytes;
    size_t dA, dB, dqkv, dprob, dctx, dhff, dpool2, dpool1, dcomb, dfused, dlogit, dpre, dh, dhb, dh2, dh3;
    size_t total;
};

// Every choice a whole-model call makes from knobs, environment variables and the plan, beyond the workspace layout (Plan: fold, flash,
// attn_b3): decided once per call by make_schedule (below, with the measurements behind each default), read by the enqueue functions,
// compared by the graph cache.  A forward call fills the forward half, a backward call the backward half; the other half stays zero.
enum { ENC_OPS = 0, ENC_ROWS, ENC_SLICED };      // encoder schedules: launch-per-op, row-fused launches, one sliced persistent launch
struct Schedule {
    bool overlap;                       // the branches on streams of their own; false: everything on the caller's stream
    int enc_fwd, enc_bwd;               // ENC_*
    // launch-per-op encoder forward: norm1 absorbed by linear1 / norm2 by the next in_proj or fingerprint_fc; out_proj -> norm1 as one
    // launch; the FFN dropout in linear1's epilogue
    bool absorb1, absorb2, ln_fused, drop_in_gemm;
    bool head_fwd_fused, head_bwd_fused;
    bool fold_bias_grad;                // backward: a bias gradient rides in its weight-gradient GEMM (linear_bwd_weight_bias)
    ConvPrefs conv1_fwd, conv2_fwd, conv2_wgrad;
    bool operator==(const Schedule& o) const {          // field by field: the structs have padding
        auto same = [](const ConvPrefs& a, const ConvPrefs& b) {
            return a.conv1_fwd_f32 == b.conv1_fwd_f32 && a.conv1_fwd_per_cu == b.conv1_fwd_per_cu && a.conv2_fwd_pipe == b.conv2_fwd_pipe && a.wgrad_beside_encoder == b.wgrad_beside_encoder;
        };
        return overlap == o.overlap && enc_fwd == o.enc_fwd && enc_bwd == o.enc_bwd && absorb1 == o.absorb1 && absorb2 == o.absorb2 && ln_fused == o.ln_fused &&
               drop_in_gemm == o.drop_in_gemm && head_fwd_fused == o.head_fwd_fused && head_bwd_fused == o.head_bwd_fused && fold_bias_grad == o.fold_bias_grad &&
               same(conv1_fwd, o.conv1_fwd) && same(conv2_fwd, o.conv2_fwd) && same(conv2_wgrad, o.conv2_wgrad);
    }
};

// Fused attention for many small heads (attention.hip); 0 selects the GEMM + softmax schedule with materialised probabilities.
Knob g_flash_attention{"BBBP_FLASH_ATTENTION", 13, [](int v) { return v & 31; }};

// out_proj folded into the value projection for one-head layers (fold.hip): two launches fewer per layer on the encoder's forward and
// backward chains.  A bit mask (default 3): bit 0 the launch-per-op schedule with materialised probabilities; bit 1 also the
// forward-only split-bf16 attention kernel of 2048+ row plans -- there the encoder alone gets faster (1.88 -> 1.76 ms at B = 4096); beside the
// conv kernels on a second stream the step measured slower with it (7.54 -> 7.79 ms; profiles/r03_fold_outproj.txt), which is one of the
// reasons those plans run on one stream (forward_enqueue).  BBBP_FOLD_OUTPROJ=0 / bbbp_set_fold_outproj(0) keep the reference's operation order.
Knob g_fold_outproj{"BBBP_FOLD_OUTPROJ", 3, [](int v) { return v & 3; }};
Knob g_fused_encoder{"BBBP_FUSED_ENCODER", 0, [](int v) { return v & 7; }};      // bit 0: row-fused kernels (opt-in); bits 1 / 2: sliced persistent forward / backward for small batches
int fold_outproj_on() { return g_fold_outproj.get(); }
// LayerNorm absorbed by the consuming Linear (gemm.hip: gemm_direct_lna_kernel).  Default OFF: measured SLOWER inside the B = 512 step
// (profiles/r04_ln_absorb.txt: the encoder's forward chain 0.826 -> 0.857 ms on the device timeline, step 2.487 -> 2.504 ms -- the absorbing
// GEMMs pay more for their row statistics / gamma / beta work beside the conv kernels than the twelve LayerNorm launches cost).
Knob g_ln_absorb{"BBBP_LN_ABSORB", 0, knob_bool};
int ln_absorb_on() { return g_ln_absorb.get(); }
int fused_encoder_mode() { return g_fused_encoder.get(); }

int make_plan(const bbbp_mixed_desc* d, Plan* p) {
    BBBP_CHECK_ARG(d, "null desc");
    BBBP_CHECK_ARG(d->batch >= 1, "batch %d < 1", d->batch);
    BBBP_CHECK_ARG(d->fingerprint_size >= 1 && d->nhead >= 1 && d->fingerprint_size % d->nhead == 0,
                   "fingerprint_size %d not divisible by nhead %d", d->fingerprint_size, d->nhead);
    BBBP_CHECK_ARG(d->num_layers >= 0 && d->num_layers <= 32, "num_layers %d not in [0, 32]", d->num_layers);
    BBBP_CHECK_ARG(d->dim_feedforward >= 1, "dim_feedforward");
    BBBP_CHECK_ARG(d->dropout_p >= 0.f && d->dropout_p < 1.f, "dropout_p %f", d->dropout_p);
    BBBP_CHECK_ARG(d->fusion == 0 || d->fusion == 1, "fusion %d (0 attention fusion, 1 concat)", d->fusion);
    BBBP_CHECK_ARG(!(d->inference && d->training), "an inference workspace cannot serve a training-mode call");
    p->concat = d->fusion == 1; p->inference = d->inference != 0;
    p->B = d->batch; p->F = d->fingerprint_size; p->NH = d->nhead; p->D = p->F / p->NH; p->L = d->num_layers;
    p->DFF = d->dim_feedforward;
    p->drop = d->training && d->dropout_p > 0.f;
    p->exact = d->collective != nullptr;
    BBBP_CHECK_ARG(p->exact || d->world <= 1, "world = %d needs a collective callback", d->world);
    p->world = p->exact && d->world > 1 ? d->world : 1; p->rank = p->exact ? d->rank : 0;
    BBBP_CHECK_ARG(p->rank >= 0 && p->rank < p->world, "rank %d of %d", d->rank, p->world);
    p->Bg = (size_t)p->B * p->world;
    const int flash_mask = g_flash_attention.get();
    // bit 3 (round 3): forward-only plans of 2048 rows and more with a wide head run the split-bf16 attention kernel (attention_b3.hip);
    // bit 4: that kernel from 256 rows on (tests; below ~2048 rows its 128-query work-groups leave most CUs idle)
    p->attn_b3 = (flash_mask & 8) && p->inference && p->L > 0 && p->B >= ((flash_mask & 16) ? 256 : 2048) &&
                 bbbp_attn_b3_supported(p->B, p->NH, p->D) && !p->exact;
    // bit 2: the wide-head kernel where it wins -- forward-only plans of 2048 rows and more (256+ work-groups fill the chip and the
    // [B, B] probability tensor, 67 MB per layer at B = 4096, is never written): config 5 8.28 -> 7.84 ms per 4096 molecules
    const bool wide = (flash_mask & 2) || ((flash_mask & 4) && p->inference && p->B >= 2048);
    p->flash = p->L > 0 && !p->exact && (p->attn_b3 || ((flash_mask & 1) && bbbp_attn_small_supported(p->B, p->NH, p->D)) ||
                            (wide && bbbp_attn_wide_supported(p->B, p->NH, p->D)));
    // the fused / sliced encoder schedules (opt-in) and the fused attention kernels keep the reference's operation order
    // (the forward-only split-bf16 attention kernel reads VW where it read V: its rows of P sum to one, so bo rides in b')
    p->fold = (((fold_outproj_on() & 1) && !p->flash) || ((fold_outproj_on() & 2) && p->attn_b3)) && p->L > 0 && !p->exact && fused_encoder_mode() == 0 &&
              bbbp_fold_supported(p->F, p->NH, p->L);
    const size_t B = p->B, F = p->F, NH = p->NH, DFF = p->DFF, Bg = p->Bg;
    Bump b;
    p->seed_slot = b.take(256);
    for (int l = 0; l < p->L; ++l) {
        LayerOff& o = p->layer[l];
        // forward only: nothing is kept for a backward pass, every layer runs in layer 0's buffers (layer l reads its input
        // y2 before it writes y2 again: qkv <- y2, y1 <- LN(z1 + y2), y2 <- LN(z2 + y1))
        // (not for batches the sliced persistent forward can take: its row blocks run layers out of step, so a layer's buffers must not be
        // the previous layer's; at B <= 128 a layer's activations are < 2 MB)
        if (p->inference && l > 0 && !bbbp_enc_sliced_supported(p->B, p->F, p->NH, p->DFF, p->L)) { o = p->layer[0]; continue; }
        o.qkv = b.f(B * 3 * F); o.prob = p->flash ? 0 : b.f(NH * B * Bg); o.ctx = b.f(B * F);
        o.kvg = p->exact ? b.f(Bg * 2 * F) : 0;          // K | V of every rank's rows, kept for the backward pass
        // dropped attention weights are KEPT per layer (1 MB at B = 512, one head) rather than recomputed in backward:
        // every launch on the encoder's chain costs more than the bytes
        o.pd = (p->drop && !p->flash) ? b.f(NH * B * Bg) : o.prob;
        o.lse = b.f(NH * B);
        // fused small-head attention with dropout: the forward pass leaves its keep decisions (one byte per lane and tile pair, 17 MB
        // per layer at F = 2048, B = 512) for the backward pass, whose dominant cost was drawing them again
        {
            const size_t kbytes = (p->flash && p->drop && !p->inference) ? bbbp_attn_small_keep_bytes(p->B, p->NH, p->D) : 0;
            o.keep = kbytes ? b.take(kbytes) : 0;          // offset 0 is the seed slot: 0 means "no mask kept"
        }
        o.z1 = b.f(B * F); o.y1 = b.f(B * F); o.hff = b.f(B * DFF); o.z2 = b.f(B * F); o.y2 = b.f(B * F);
        o.mean1 = b.f(B); o.rstd1 = b.f(B); o.mean2 = b.f(B); o.rstd2 = b.f(B);
    }
    if (p->L > 0 && bbbp_enc_sliced_supported(p->B, p->F, p->NH, p->DFF, p->L)) {
        p->sl_sync = b.take(bbbp_enc_sliced_sync_bytes());
        p->sl_part = b.take(bbbp_enc_sliced_part_bytes(p->B, p->F));
        p->sl_kvpart = p->inference ? 0 : b.take(bbbp_enc_sliced_kvpart_bytes(p->B, p->F));
    } else {
        p->sl_sync = p->sl_part = p->sl_kvpart = 0;
    }
    for (int l = 0; l < p->L; ++l) {
        p->fwf[l] = p->fold ? b.f(bbbp_outproj_fold_floats(p->F, 0)) : 0; p->fbf[l] = p->fold ? b.f(bbbp_outproj_fold_floats(p->F, 1)) : 0;
        p->fwvt[l] = p->fold ? b.f(bbbp_outproj_fold_floats(p->F, 2)) : 0;
        p->ftdw[l] = (p->fold && !p->inference) ? b.f(bbbp_outproj_fold_floats(p->F, 3)) : 0;
        p->ftdb[l] = (p->fold && !p->inference) ? b.f(bbbp_outproj_fold_floats(p->F, 4)) : 0;
    }
    p->attn_part_bytes = p->attn_b3 ? bbbp_attn_b3_workspace_bytes(p->B, p->NH, p->D) : 0;
    p->attn_part = p->attn_part_bytes ? b.take(p->attn_part_bytes) : 0;
    // forward-only plans keep NO pooling decisions (nothing reads them: 0.8 GB per step at B = 4096): offset 0 = "no mask"
    p->pool1 = b.f(B * C1 * (IMG / 2) * (IMG / 2)); p->mask1 = p->inference ? 0 : b.take(B * C1 * (IMG / 2) * (IMG / 2));
    p->pool2 = b.f(B * IMG_FLAT); p->mask2 = p->inference ? 0 : b.take(B * IMG_FLAT);
    p->combined = b.f(B * COMB); p->hid = b.f(NHEADS_FUSION * B * FUS_HID); p->attn = b.f(B * NHEADS_FUSION);
    p->fused = p->concat ? p->combined : b.f(B * COMB); p->h = b.f(B * H1); p->hb = b.f(B * H1); p->bn_mean = b.f(H1); p->bn_rstd = b.f(H1);
    p->h2 = b.f(B * H2); p->h3 = b.f(B * H3);
    p->head_partial = b.f((size_t)p->world * ((B + 15) / 16) * 2 * H1);
    size_t cw = bbbp_conv3x3_workspace_bytes(p->B, 32, 64, 64, 64);
    size_t cw1 = bbbp_conv3x3_workspace_bytes(p->B, 3, 32, 128, 128);
    size_t sb = cw > cw1 ? cw : cw1;
    size_t gw = bbbp_gemm_workspace_bytes(p->B, FC, IMG_FLAT, 1);
    if (gw > sb) sb = gw;
    if (sb < ((size_t)32 << 20)) sb = (size_t)32 << 20;
    p->scratch_bytes = sb;
    p->scratch = b.take(sb);
    // the fingerprint branch runs on its own stream beside the image branch: it needs its own split-K scratch
    p->scratch2_bytes = (size_t)32 << 20;
    p->scratch2 = b.take(p->scratch2_bytes);
    if (p->inference) { p->total = b.off; return BBBP_OK; }
    // backward temporaries
    for (int l = 0; l < p->L; ++l) {
        LayerGrad& g = p->lgrad[l];
        g.dyout = b.f(B * F); g.dz2 = b.f(B * F); g.dz2d = p->drop ? b.f(B * F) : g.dz2; g.dhff = b.f(B * DFF);
        g.dy1 = b.f(B * F); g.dz1 = b.f(B * F); g.dz1d = p->drop ? b.f(B * F) : g.dz1; g.dqkv = b.f(B * 3 * F);
    }
    p->scratch3_bytes = (size_t)32 << 20;
    p->scratch3 = b.take(p->scratch3_bytes);
    p->dA = b.f(B * F); p->dB = b.f(B * F); p->dqkv = b.f(B * 3 * F); p->dprob = p->flash ? 0 : b.f(NH * B * Bg); p->dctx = b.f(B * F);
    p->dkvg = p->exact ? b.f(Bg * 2 * F) : 0; p->dkvl = p->exact ? b.f(B * 2 * F) : 0;
    p->dhff = b.f(B * DFF); p->dpool2 = b.f(B * IMG_FLAT); p->dpool1 = b.f(B * C1 * (IMG / 2) * (IMG / 2));
    p->dcomb = b.f(B * COMB); p->dfused = b.f(B * COMB); p->dlogit = b.f(NHEADS_FUSION * B);
    p->dpre = b.f(NHEADS_FUSION * B * FUS_HID); p->dh = b.f(B * H1); p->dhb = b.f(B * H1); p->dh2 = b.f(B * H2);
    p->dh3 = b.f(B * H3);
    p->total = b.off;
    return BBBP_OK;
}

// exact-global-batch mode: K | V of this rank's rows into its slot of the gathered buffer, and the reduce-scattered dK | dV back into dqkv
__global__ __launch_bounds__(256) void kv_pack_kernel(const float* __restrict__ qkv, float* __restrict__ kv, long n, int F) {
    BBBP_HIGH_PRIO();
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) { const long r = i / (2 * F); const int c = (int)(i % (2 * F)); kv[i] = qkv[r * 3 * F + F + c]; }
}
__global__ __launch_bounds__(256) void kv_unpack_kernel(const float* __restrict__ dkv, float* __restrict__ dqkv, long n, int F) {
    BBBP_HIGH_PRIO();
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) { const long r = i / (2 * F); const int c = (int)(i % (2 * F)); dqkv[r * 3 * F + F + c] = dkv[i]; }
}
int run_collective(const bbbp_mixed_desc* d, int op, int what, int layer, size_t send_off, size_t recv_off, size_t count, hipStream_t st) {
    BBBP_CHECK_ARG(d->collective, "no collective callback");
    const int rc = d->collective(d->collective_ctx, op, what, layer, send_off, recv_off, count, st);
    if (rc) { bbbp_set_error("collective callback (op %d, what %d, layer %d) returned %d", op, what, layer, rc); return BBBP_ERR_ARG; }
    return BBBP_OK;
}

#define TRY(expr) do { int _rc = (expr); if (_rc) return _rc; } while (0)

struct Ctx {
    hipStream_t st;
    char* ws;
    const Plan* p;
    const Schedule* s;
    int side = 0;         // 0 main stream, 1 fingerprint-branch chain, 2 weight-gradient leaves: own scratch each
    float* f(size_t off) const { return reinterpret_cast<float*>(ws + off); }
    uint8_t* u8(size_t off) const { return reinterpret_cast<uint8_t*>(ws + off); }
    void* scratch() const { return ws + (side == 0 ? p->scratch : side == 1 ? p->scratch2 : p->scratch3); }
    size_t scratch_bytes() const { return side == 0 ? p->scratch_bytes : side == 1 ? p->scratch2_bytes : p->scratch3_bytes; }
};

// ---- two-branch overlap -------------------------------------------------------------------------
// The fingerprint branch (encoder, F = 167: ~270 launches of a few microseconds each, latency-bound) and the image
// branch (five persistent MFMA-bound conv kernels) are independent between the input and the fusion block.  They
// are enqueued on two HIP streams (fork/join with events, graph-capturable) so the small kernels run in the shadow
// of the conv kernels: their work-groups are sized to co-reside on a CU with a conv work-group.
constexpr int NEV = 32;
struct SideStream { hipStream_t s = nullptr; hipStream_t leaf = nullptr; hipEvent_t fork = nullptr, join = nullptr, join2 = nullptr;
                    hipEvent_t ev[NEV]; int next = 0; };
// A gradient bucket's event and whether the most recent backward pass on the device recorded it (bbbp_mixed_backward_wait_bucket)
struct BucketEvent { hipEvent_t ev = nullptr; bool recorded = false; };
struct DeviceState {
    SideStream side;
    // recorded on the caller's stream when the image-FC weight gradient (33.5 MB of the 53.9 MB of gradients at F = 167) is
    // final, i.e. after the first GEMM of the image branch's backward: a data-parallel caller can start reducing that bucket
    // while the remaining ~2 ms of the backward pass run
    BucketEvent bucket0;
    BucketEvent bucket0_released;      // recorded after the last READ of the image-FC weight in a backward pass, only on request (g_release_events)
    // bucket 1: everything except the image-FC weight and the four conv tensors -- final when the fingerprint branch's chain
    // and all weight-gradient leaves are done (~0.25 ms before the image branch's last kernel); recorded on the leaf stream
    BucketEvent bucket1;
    // buckets 2 + l: the twelve tensors of encoder layer l (one contiguous slice in named_parameters order) -- final when that
    // layer's weight-gradient leaves are, layer L-1 first.  At F = 2048 these are 100 MB each and 94 % of all gradient bytes.
    BucketEvent layer[32];
};
DeviceState g_device[64];
bool g_release_events = false;          // bbbp_set_release_events: one more record on the image branch's stream
// the current device's record (and its index); nullptr for a device beyond the table: the callers skip their events then, or report it
int device_state(DeviceState** out, int* dev_out = nullptr) {
    int dev = 0;
    BBBP_CHECK_HIP(hipGetDevice(&dev));
    if (dev_out) *dev_out = dev;
    *out = (dev >= 0 && dev < 64) ? &g_device[dev] : nullptr;
    return BBBP_OK;
}
// record bucket `b` (created at first use) as final at this point of `st`
int record_bucket(BucketEvent& b, hipStream_t st) {
    if (!b.ev) BBBP_CHECK_HIP(hipEventCreateWithFlags(&b.ev, hipEventDisableTiming));
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    (void)hipStreamIsCapturing(st, &cap);
    b.recorded = cap == hipStreamCaptureStatusNone;       // an event recorded inside a graph capture means nothing outside it
    if (b.recorded) BBBP_CHECK_HIP(hipEventRecord(b.ev, st));
    return BBBP_OK;
}
int g_overlap = -1;
Knob g_fused_head_bwd{"BBBP_FUSED_HEAD_BWD", 1, knob_bool};
// Row-local stretches of an encoder layer as single launches (encoder.hip) instead of 6 + 6 per layer: BBBP_FUSED_ENCODER=1 /
// bbbp_set_fused_encoder(1).  Correct (tests compare the two schedules) but OFF by default: a 16-row work-group streams a whole
// layer's weights by itself (3.2 MB forward) through ONE wave per SIMD, which is bound by load latency -- 176 / 289 us per
// forward / backward launch against ~50 us for the launch-per-op chain whose GEMMs spread over all CUs.
bool fused_encoder(const Plan& p) {
    return (fused_encoder_mode() & 1) && p.L > 0 && !p.flash && !p.exact && bbbp_enc_rows_supported(p.F, p.NH, p.DFF);
}
// the whole forward chain of a small batch as one persistent launch (encoder.hip: enc_sliced_fwd_kernel)
bool sliced_encoder(const Plan& p, int bit = 2) {
    return (fused_encoder_mode() & bit) && p.L > 0 && !p.flash && !p.exact && bbbp_enc_sliced_supported(p.B, p.F, p.NH, p.DFF, p.L);
}
bool overlap_enabled() {
    if (g_overlap < 0) { const char* e = bbbp_env("BBBP_SINGLE_STREAM"); g_overlap = (e && e[0] == '1') ? 0 : 1; }
    return g_overlap == 1;
}
int reserved_cus() {
    // default 0: measured (tools/exp_overlap.py, bench sweeps) the reservation costs the conv kernels what it gives
    static const int v = bbbp_env_int("BBBP_RESERVED_CUS", 0);
    return (v < 0 || v > 128) ? 0 : v;
}
// scoped CU partition (common.h): conv grids leave `reserved_cus()` CUs to the side stream's small kernels
// The Winograd conv2 kernels take a whole CU each (496 registers per lane, 110-154 KB LDS): nothing of the side stream
// can start beside them, so while the branches overlap their grids leave `wino_side_cus()` CUs entirely to the side
// stream.  Measured (tools/exp_wino.sh, ms/step): 256 CUs 3.65, 224 3.51, 192 3.42, 160 3.51, 128 3.76.
int wino_side_cus() {
    static const int v = bbbp_env_int("BBBP_WINO_SIDE_CUS", 64);
    return (v < 0 || v > 192) ? 64 : v;
}
struct Partition {
    bool on, side;
    explicit Partition(bool enable) : on(enable && reserved_cus() > 0), side(enable) {
        if (on) { g_bbbp_reserved_cus = reserved_cus(); g_bbbp_small_lds_pad = 48 * 1024; }
        if (side) g_bbbp_wino_side_cus = wino_side_cus();
    }
    ~Partition() {
        if (on) { g_bbbp_reserved_cus = 0; g_bbbp_small_lds_pad = 0; }
        if (side) g_bbbp_wino_side_cus = 0;
    }
};
// An environment-only knob is read once per process, at the first call of its direction; a knob with a setter again at every call.
Schedule make_schedule(const Plan& p, bool backward) {
    Schedule s{};
    const int B = p.B, F = p.F, DFF = p.DFF;
    if (backward) {
        s.overlap = overlap_enabled();          // (a training plan is never a screening plan)
        // (the backward kernel takes bit 2 of the mode and its own share of the workspace)
        s.enc_bwd = (sliced_encoder(p, 4) && p.sl_sync && p.sl_kvpart) ? ENC_SLICED : fused_encoder(p) ? ENC_ROWS : ENC_OPS;
        // default ON since round 2 (bbbp_set_fused_head_bwd / BBBP_FUSED_HEAD_BWD=0 select the launch-per-op chain): with the bias
        // gradients folded into the weight-gradient GEMMs the leaves it feeds are short enough that the shorter chain shows --
        // B = 512 3.32 -> 3.27 ms, B = 256 2.12 -> 2.08, B = 128 2.36 -> 2.23 (round 1, with 38 separate column-sum leaves: neutral)
        s.head_bwd_fused = g_fused_head_bwd.get() && !p.concat;
        static const int fold_bias = bbbp_env_int("BBBP_FOLD_BIAS_GRAD", 1);
        s.fold_bias_grad = fold_bias != 0;
        // beside the encoder's backward chain the sparse weight-gradient kernel runs one wave per SIMD (common.h); the rule looks at the
        // plan only, not at the stream mode: one stream or three give bit-identical steps
        s.conv2_wgrad.wgrad_beside_encoder = p.L > 0 ? 1 : 0;
        return s;
    }
    // Screening plans (forward-only, 2048+ rows on the bf16 attention kernel) run on ONE stream: there both branches are bound by the matrix
    // pipe, so the second stream only time-shares it -- measured equal on one box (6.66 / 6.83 ms overlapped, 6.59 / 6.85 one stream) and
    // WORSE than the sum of the branches on others (7.6 ms against 5.29 + 1.85 + 0.06; profiles/r03_config5_streams.txt); alone, the
    // encoder also takes the out_proj fold's gain (fold mask bit 1).  BBBP_SCREEN_OVERLAP=1 restores the two-stream schedule.
    static const bool screen_overlap = bbbp_env_int("BBBP_SCREEN_OVERLAP", 0) != 0;
    s.overlap = overlap_enabled() && (screen_overlap || !p.attn_b3);
    s.enc_fwd = (sliced_encoder(p) && p.sl_sync) ? ENC_SLICED : fused_encoder(p) ? ENC_ROWS : ENC_OPS;
    const bool beside_chain = !p.inference && p.L > 0;
    // conv1: beside a training step's encoder chain the f32 form stays (common.h: ConvPrefs::conv1_fwd_f32); screening batches, eval loops and
    // the encoder-less two-branch model take the split-bf16 form when the conv mask selects it (bit 6, default)
    // (the rule looks at the plan only, not at the stream mode: one stream or three give bit-identical steps)
    // round 4: training steps run the software-pipelined split-bf16 kernel (conv_b3c1.hip) too, ONE work-group per CU beside the chain
    // (BBBP_C1_TRAIN=0: the f32 kernel of rounds 1-3 there; 2: two work-groups per CU, measured slower for the step)
    static const int c1_train = bbbp_env_int("BBBP_C1_TRAIN", 1);      // default 1: step 2.517 -> 2.487 ms (profiles/r04_c1_pipe.txt)
    s.conv1_fwd.conv1_fwd_f32 = (beside_chain && !c1_train) ? 1 : 0;
    s.conv1_fwd.conv1_fwd_per_cu = (beside_chain && c1_train) ? (c1_train >= 2 ? 2 : 1) : 0;      // BBBP_C1_TRAIN=2: two work-groups per CU there too
    // conv2, round 4: beside a training step's encoder chain the software-pipelined one-work-group-per-CU kernel (conv_b3.hip): 0.40 instead of
    // 0.387 ms alone, but the chain -- the forward half's critical path -- keeps three quarters of every SIMD: step 2.41 -> 2.34 ms
    // (profiles/r04_conv2_pipe.txt).  BBBP_C2_TRAIN=0: the two-work-group kernel there too.  Bit-identical outputs either way.
    static const int c2_train = bbbp_env_int("BBBP_C2_TRAIN", 1);
    s.conv2_fwd.conv2_fwd_pipe = (beside_chain && c2_train) ? 1 : 0;
    // LayerNorm absorbed by the Linear that consumes it (BBBP_LN_ABSORB=0 keeps the stand-alone launches; Step::encoder_layer_fwd_ops)
    const bool lna_ok = ln_absorb_on() && s.enc_fwd == ENC_OPS && !p.exact && p.L > 0 && bbbp_layernorm_linear_preferred(B, DFF, F) &&
                        bbbp_layernorm_linear_preferred(B, 3 * F, F) && bbbp_layernorm_linear_preferred(B, FC, F) &&
                        // training: the producers' dropout rides in the small-product GEMM's epilogue only
                        (!p.drop || (bbbp_gemm_folds_asum(B, F, DFF, 1) && bbbp_gemm_folds_asum(B, F, p.fold ? (int)p.Bg : F, 1)));
    s.absorb1 = lna_ok && !(p.attn_b3 && p.fold);      // (that attention kernel writes z1 itself: no epilogue for the residual)
    s.absorb2 = lna_ok;
    // out_proj -> (dropout) + residual -> norm1 as one launch (gemm.hip: gemm_direct_ln_kernel).
    // OPT-IN (BBBP_FUSED_LINEAR_LN=1), measured slower at B = 512: the 11-wave work-groups need three wave slots on three SIMDs of a CU
    // beside the resident conv work-groups (encoder forward 0.98 -> 1.15 ms in the step, 0.58 -> 0.60 alone); linear2 -> norm2 is never
    // fused (one wave per tile walking K = 2048 alone: 90 us against 22 + 4)
    static const bool ln_opt_in = bbbp_env_int("BBBP_FUSED_LINEAR_LN", 0) != 0;
    s.ln_fused = s.enc_fwd == ENC_OPS && !p.fold && ln_opt_in && bbbp_linear_layernorm_supported(B, F, F) && F <= 512;
    s.drop_in_gemm = s.enc_fwd == ENC_OPS && p.drop && bbbp_gemm_folds_asum(B, DFF, F, 1);
    static const int fused_head = bbbp_env_int("BBBP_FUSED_HEAD", 1);
    s.head_fwd_fused = fused_head && NHEADS_FUSION == 4;
    return s;
}

int get_side(SideStream** out) {
    DeviceState* ds = nullptr; int dev = 0;
    TRY(device_state(&ds, &dev));
    BBBP_CHECK_ARG(ds, "device index %d", dev);
    SideStream& ss = ds->side;
    if (!ss.s) {
        // (queue priorities -- hipStreamCreateWithPriority, chain stream highest / leaf stream lowest -- were measured on the headline step:
        // 2.497 ms default, 2.501 / 2.508 with them, profiles/r03_rebalance.txt; the wave priority set inside the kernels is what matters)
        BBBP_CHECK_HIP(hipStreamCreateWithFlags(&ss.s, hipStreamNonBlocking));
        BBBP_CHECK_HIP(hipEventCreateWithFlags(&ss.fork, hipEventDisableTiming));
        BBBP_CHECK_HIP(hipEventCreateWithFlags(&ss.join, hipEventDisableTiming));
        BBBP_CHECK_HIP(hipStreamCreateWithFlags(&ss.leaf, hipStreamNonBlocking));
        BBBP_CHECK_HIP(hipEventCreateWithFlags(&ss.join2, hipEventDisableTiming));
        for (int i = 0; i < NEV; ++i) BBBP_CHECK_HIP(hipEventCreateWithFlags(&ss.ev[i], hipEventDisableTiming));
    }
    *out = &ss;
    return BBBP_OK;
}
int fork_side(hipStream_t main, SideStream* ss) {
    BBBP_CHECK_HIP(hipEventRecord(ss->fork, main));
    BBBP_CHECK_HIP(hipStreamWaitEvent(ss->s, ss->fork, 0));
    return BBBP_OK;
}
// make stream `waiter` wait for everything enqueued so far on stream `producer`
int after(SideStream* ss, hipStream_t producer, hipStream_t waiter) {
    if (producer == waiter) return BBBP_OK;
    hipEvent_t e = ss->ev[ss->next];
    ss->next = (ss->next + 1) % NEV;
    BBBP_CHECK_HIP(hipEventRecord(e, producer));
    BBBP_CHECK_HIP(hipStreamWaitEvent(waiter, e, 0));
    return BBBP_OK;
}
int join_side(hipStream_t main, SideStream* ss) {
    BBBP_CHECK_HIP(hipEventRecord(ss->join, ss->s));
    BBBP_CHECK_HIP(hipStreamWaitEvent(main, ss->join, 0));
    return BBBP_OK;
}

// ---- optional per-section timing with HIP events on the launch stream (bench.py roofline leg) ----
enum { SEC_CONV1_FWD = 0, SEC_CONV2_FWD, SEC_IMGFC_FWD, SEC_ENCODER_FWD, SEC_HEAD_FWD, SEC_HEAD_BWD, SEC_IMGFC_BWD,
       SEC_CONV2_WGRAD, SEC_CONV2_DGRAD, SEC_CONV1_WGRAD, SEC_ENCODER_BWD, SEC_FFN1_FWD, SEC_FFN2_FWD,
       // the other per-layer kernels of the launch-per-op encoder schedule (one instance per layer and step): chain ...
       SEC_QKV_FWD, SEC_ATTN_FWD, SEC_OUTPROJ_FWD, SEC_LN_FWD, SEC_LN_BWD, SEC_FFN2_DGRAD, SEC_FFN1_DGRAD, SEC_OUTPROJ_DGRAD, SEC_ATTN_BWD,
       SEC_QKV_DGRAD,
       // ... and weight-gradient leaves (leaf stream)
       SEC_FFN2_WGRAD, SEC_FFN1_WGRAD, SEC_OUTPROJ_WGRAD, SEC_QKV_WGRAD, SEC_COUNT };
static_assert(SEC_COUNT <= 32, "bbbp_profile_select takes a 32-bit mask");
const char* const kSectionNames[SEC_COUNT] = {"conv1_fwd", "conv2_fwd", "imgfc_fwd", "encoder_fwd", "head_fwd", "head_bwd",
                                              "imgfc_bwd", "conv2_wgrad", "conv2_dgrad", "conv1_wgrad", "encoder_bwd",
                                              "ffn1_fwd", "ffn2_fwd",          // the encoder's two FFN GEMMs, one instance per layer
                                              "qkv_fwd", "attn_fwd", "outproj_fwd", "ln_fwd", "ln_bwd", "ffn2_dgrad", "ffn1_dgrad",
                                              "outproj_dgrad", "attn_bwd", "qkv_dgrad", "ffn2_wgrad", "ffn1_wgrad", "outproj_wgrad",
                                              "qkv_wgrad"};
constexpr int PROF_MAX = 16384;
struct ProfState {
    bool on = false;
    unsigned mask = ~0u;          // sections that record events (bbbp_profile_select)
    int n = 0;
    int sec[PROF_MAX];
    hipEvent_t a[PROF_MAX], b[PROF_MAX];
    int created = 0;
} g_prof;

struct Section {
    hipStream_t st; int idx;
    Section(hipStream_t s, int sec) : st(s), idx(-1) {          // sec < 0: no section
        if (sec < 0 || !g_prof.on || !((g_prof.mask >> sec) & 1u) || g_prof.n >= PROF_MAX) return;
        idx = g_prof.n++;
        if (idx >= g_prof.created) {
            if (hipEventCreate(&g_prof.a[idx]) != hipSuccess || hipEventCreate(&g_prof.b[idx]) != hipSuccess) { idx = -1; --g_prof.n; return; }
            g_prof.created = idx + 1;
        }
        g_prof.sec[idx] = sec;
        (void)hipEventRecord(g_prof.a[idx], st);
    }
    ~Section() { if (idx >= 0) (void)hipEventRecord(g_prof.b[idx], st); }
};

// y[M,N] = act(x[M,K] W[N,K]^T + b) + res
int linear_fwd(const Ctx& c, const float* x, int ldx, const float* W, const float* b, float* y, int ldy, int M, int N, int K,
               int act, const float* res = nullptr, int ldr = 0) {
    return bbbp_gemm_f32(c.st, 0, 1, M, N, K, 1.f, x, ldx, W, K, y, ldy, b, res, ldr, act, 1, 0, 0, 0, 0, c.scratch(),
                         c.scratch_bytes());
}
// dx[M,K] = dy[M,N] W[N,K] + res
int linear_bwd_input(const Ctx& c, const float* dy, int lddy, const float* W, float* dx, int lddx, int M, int N, int K,
                     const float* res = nullptr, int ldr = 0) {
    return bbbp_gemm_f32(c.st, 0, 0, M, K, N, 1.f, dy, lddy, W, K, dx, lddx, nullptr, res, ldr, 0, 1, 0, 0, 0, 0, c.scratch(),
                         c.scratch_bytes());
}
// dW[N,K] = dy[M,N]^T x[M,K]
int linear_bwd_weight(const Ctx& c, const float* dy, int lddy, const float* x, int ldx, float* dW, int M, int N, int K) {
    return bbbp_gemm_f32(c.st, 1, 0, N, K, M, 1.f, dy, lddy, x, ldx, dW, K, nullptr, nullptr, 0, 0, 1, 0, 0, 0, 0, c.scratch(),
                         c.scratch_bytes());
}

bbbp_gemm_desc gemm_desc(int transA, int transB, int M, int N, int K, float alpha, const float* A, int lda, const float* B, int ldb,
                         float* C, int ldc, int batch = 1, long sA = 0, long sB = 0, long sC = 0) {
    bbbp_gemm_desc g;
    g.transA = transA; g.transB = transB; g.M = M; g.N = N; g.K = K; g.alpha = alpha;
    g.A = A; g.lda = lda; g.B = B; g.ldb = ldb; g.C = C; g.ldc = ldc;
    g.bias = nullptr; g.residual = nullptr; g.ldr = 0; g.act = 0; g.gate = nullptr; g.ldg = 0; g.gate_scale = 1.f;
    g.gate_after_residual = 0; g.asum = nullptr; g.drop_p = 0.f; g.drop_seed = 0;
    g.batch = batch; g.strideA = sA; g.strideB = sB; g.strideC = sC; g.strideR = 0; g.strideG = 0;
    return g;
}
// dW[N,K] = dy[M,N]^T x[M,K] and db[N] = column sums of dy: ONE launch when the product takes the small-GEMM path (the bias
// gradient rides through the same MFMAs as a virtual all-ones column of x), else the GEMM plus a column-sum kernel
int linear_bwd_weight_bias(const Ctx& c, const float* dy, int lddy, const float* x, int ldx, float* dW, float* db, int M, int N, int K) {
    if (c.s->fold_bias_grad && bbbp_gemm_folds_asum(N, K, M, 1)) {
        bbbp_gemm_desc g = gemm_desc(1, 0, N, K, M, 1.f, dy, lddy, x, ldx, dW, K, 1, 0, 0, 0);
        g.asum = db;
        return bbbp_gemm_f32_grouped(c.st, &g, 1, c.scratch(), c.scratch_bytes());
    }
    TRY(linear_bwd_weight(c, dy, lddy, x, ldx, dW, M, N, K));
    return bbbp_bias_act_bwd(c.st, const_cast<float*>(dy), lddy, nullptr, 0, db, M, N, 0, 1.f);
}

// per-site salt; the kernels mix it with the call's seed read from device memory (effective_seed)
uint64_t site_seed(int layer, int site) { return (uint64_t)(layer * 8 + site + 1); }

__global__ void set_seed_kernel(unsigned long long* slot, unsigned long long seed) { *slot = seed; }

struct SeedScope {
    const unsigned long long* prev;
    explicit SeedScope(const unsigned long long* slot) : prev(g_bbbp_seed_base) { g_bbbp_seed_base = slot; }
    ~SeedScope() { g_bbbp_seed_base = prev; }        // (the op-level base a caller set with bbbp_set_seed_base survives a whole-model call)
};

// ---- HIP-graph replay of the two whole-model calls ---------------------------------------------------------------
// A call enqueues 85 (forward) or 175 (backward) launches plus ~100 event operations: ~0.5 / 0.9 ms of host time.  For
// fixed arguments the enqueued work is identical from step to step (the dropout seed is read from device memory), so
// the second time a call arrives with the same arguments its enqueue is captured (all three streams: the fork/join
// events pull the side streams into the capture) and from then on replayed with one hipGraphLaunch.  Anything that
// changes an argument (another batch tensor, re-flattened parameters, a different batch size) is a different key;
// the cache holds a few entries, least recently used first out.  So is a knob set to another value: the key holds what was decided from
// the knobs (the schedule, and the plan's choices that move workspace offsets).  Opt-in (see graphs_mode); section profiling bypasses it.
struct GraphKey {
    int kind;                      // 0 forward, 1 backward
    bbbp_mixed_desc d;             // every field make_plan reads but the seed (collective calls never get here)
    const void* ptr[6];
    uint64_t phash;                // hash of the parameter / gradient / BN pointer arrays
    Schedule s;
    bool fold, flash, attn_b3; size_t total;      // of the plan
    hipStream_t st;
    bool operator==(const GraphKey& o) const {
        return kind == o.kind && d.batch == o.d.batch && d.fingerprint_size == o.d.fingerprint_size && d.nhead == o.d.nhead &&
               d.num_layers == o.d.num_layers && d.dim_feedforward == o.d.dim_feedforward && d.training == o.d.training &&
               d.dropout_p == o.d.dropout_p && d.need_input_grad == o.d.need_input_grad && d.inference == o.d.inference &&
               d.fusion == o.d.fusion && d.world == o.d.world && d.rank == o.d.rank && phash == o.phash && s == o.s && fold == o.fold &&
               flash == o.flash && attn_b3 == o.attn_b3 && total == o.total && st == o.st && ptr[0] == o.ptr[0] && ptr[1] == o.ptr[1] &&
               ptr[2] == o.ptr[2] && ptr[3] == o.ptr[3] && ptr[4] == o.ptr[4] && ptr[5] == o.ptr[5];
    }
};
struct GraphEntry { GraphKey key; hipGraphExec_t exec = nullptr; unsigned long long stamp = 0; bool seen_only = true; };
constexpr int GRAPH_SLOTS = 12;
GraphEntry g_graphs[GRAPH_SLOTS];
unsigned long long g_graph_clock = 0;
long g_graph_replays = 0, g_graph_captures = 0;

// Default OFF: on ROCm 7.2 replaying the captured three-stream graph is SLOWER on the GPU than the hand-scheduled
// streams (whole step, B = 512: 3.67 ms eager, 4.50 ms replayed; the host loop is not shorter either, hipGraphLaunch of
// a 260-node graph costs about what the eager enqueue does).  Kept as an opt-in (BBBP_GRAPHS=1 / bbbp_set_graphs) with a
// bit-exactness test, for runtimes where graph launch is cheaper.
int g_graphs_mode = -1;          // BBBP_GRAPHS is taken as it stands; the setter stores 0 / 1
int graphs_mode() {
    if (g_graphs_mode < 0) g_graphs_mode = bbbp_env_int("BBBP_GRAPHS", 0);
    return g_graphs_mode;
}
uint64_t hash_ptrs(const void* const* a, int n, uint64_t h = 1469598103934665603ull) {
    for (int i = 0; i < n; ++i) { h ^= (uint64_t)reinterpret_cast<uintptr_t>(a[i]); h *= 1099511628211ull; }
    return h;
}
// 0: run eagerly; 1: capture now into *slot; 2: replay *slot
int graph_lookup(const GraphKey& k, GraphEntry** slot) {
    if (!graphs_mode() || g_prof.on) return 0;
    ++g_graph_clock;
    GraphEntry* lru = &g_graphs[0];
    for (auto& e : g_graphs) {
        if (e.stamp && e.key == k) {
            e.stamp = g_graph_clock; *slot = &e;
            return e.seen_only ? 1 : 2;
        }
        if (e.stamp < lru->stamp) lru = &e;
    }
    if (lru->exec) { (void)hipGraphExecDestroy(lru->exec); lru->exec = nullptr; }
    lru->key = k; lru->stamp = g_graph_clock; lru->seen_only = true;       // first sighting: eager
    return 0;
}

}  // namespace

// Branch overlap on/off at run time (default on; env BBBP_SINGLE_STREAM=1 starts with it off).  Returns the old value.
extern "C" int bbbp_set_fused_head_bwd(int on) {
    const int prev = g_fused_head_bwd.v > 0 ? 1 : 0;          // (0 until the knob has been read or set, as it always was)
    g_fused_head_bwd.v = on ? 1 : 0;
    return prev;
}
extern "C" int bbbp_set_fused_encoder(int mode) { return g_fused_encoder.set(mode); }
extern "C" int bbbp_set_fold_outproj(int on) { return g_fold_outproj.set(on); }
extern "C" int bbbp_set_flash_attention(int on) { return g_flash_attention.set(on); }
extern "C" int bbbp_set_ln_absorb(int on) { return g_ln_absorb.set(on); }

extern "C" int bbbp_set_overlap(int on) { int old = overlap_enabled() ? 1 : 0; g_overlap = on ? 1 : 0; return old; }

// Profiling: enable, run steps, synchronise the stream, then collect {sum of ms, launches} per section.
extern "C" int bbbp_profile_enable(int on) { g_prof.on = on != 0; g_prof.n = 0; return BBBP_OK; }
extern "C" int bbbp_profile_select(unsigned section_mask) { g_prof.mask = section_mask ? section_mask : ~0u; return BBBP_OK; }
extern "C" int bbbp_profile_num_sections(void) { return SEC_COUNT; }
extern "C" const char* bbbp_profile_section_name(int i) { return (i >= 0 && i < SEC_COUNT) ? kSectionNames[i] : ""; }
extern "C" int bbbp_profile_collect(float* ms_sum, int* count) {
    for (int i = 0; i < SEC_COUNT; ++i) { ms_sum[i] = 0.f; count[i] = 0; }
    for (int i = 0; i < g_prof.n; ++i) {
        float ms = 0.f;
        BBBP_CHECK_HIP(hipEventElapsedTime(&ms, g_prof.a[i], g_prof.b[i]));
        ms_sum[g_prof.sec[i]] += ms;
        count[g_prof.sec[i]] += 1;
    }
    g_prof.n = 0;
    return BBBP_OK;
}

// Absolute placement of the recorded section instances (does not clear them): start / end in ms after the first instance's
// start.  Events of different streams share the device timeline, so the gaps between sections are visible.
extern "C" int bbbp_profile_timeline(int* section, float* start_ms, float* end_ms, int max_entries) {
    BBBP_CHECK_ARG(section && start_ms && end_ms && max_entries >= 0, "profile_timeline: bad arguments");
    const int n = g_prof.n < max_entries ? g_prof.n : max_entries;
    for (int i = 0; i < n; ++i) {
        section[i] = g_prof.sec[i];
        BBBP_CHECK_HIP(hipEventElapsedTime(&start_ms[i], g_prof.a[0], g_prof.a[i]));
        BBBP_CHECK_HIP(hipEventElapsedTime(&end_ms[i], g_prof.a[0], g_prof.b[i]));
    }
    return n;
}

extern "C" int bbbp_mixed_num_params(const bbbp_mixed_desc* d) {
    if (!d) return -1;
    if (d->num_layers < 0 || d->num_layers > 32 || (d->fusion != 0 && d->fusion != 1)) return -1;
    return PIdx(d).count();
}

extern "C" size_t bbbp_mixed_workspace_bytes(const bbbp_mixed_desc* d) {
    Plan p;
    if (make_plan(d, &p)) return 0;
    return p.total;
}

namespace {

// the absorbed LayerNorm that the next Linear of the launch-per-op forward chain still has to apply (z == nullptr: none)
struct PendingNorm { const float* z = nullptr; const float* gamma = nullptr; const float* beta = nullptr; float* y = nullptr; float* mean = nullptr; float* rstd = nullptr; };

// One whole-model call: what every part of the step reads.  `c` (the caller's stream) carries the image branch, the fusion block and the
// head; `ce` the fingerprint branch's dependency chain; `cl` (backward only) the LEAVES -- weight and bias gradients, LayerNorm parameter
// gradients -- which nothing downstream waits for, so the chain's critical path is half as long.  Without overlap all three are the
// caller's stream.  `plan`: made from `d` and checked against the arguments and the workspace size by the caller (bbbp_mixed_forward).
struct Step {
    const bbbp_mixed_desc* d; const Plan& plan; const Schedule& s; const float* const* P; float* const* G;
    const float* fingerprint; const float* image;
    const PIdx ix;
    Ctx c, ce, cl;
    SideStream* ss = nullptr; DeviceState* ds = nullptr;          // ds: this device's gradient-bucket events (backward)
    const int B, F, NH, D, DFF;
    const int Bk;                       // attention keys: this rank's rows, or every rank's in exact-global-batch mode
    const float p_drop, inv_keep, scale;
    float *comb, *hid, *fused, *h, *hb, *h2, *h3;
    float *dh3 = nullptr, *dh2 = nullptr, *dhb = nullptr, *dh = nullptr, *dfused = nullptr, *dcomb = nullptr, *dlogit = nullptr, *dpre = nullptr;

    Step(void* stream, const bbbp_mixed_desc* desc, const Plan& pl, const Schedule& sc, const float* const* params, float* const* grads,
         const float* fp, const float* img, void* workspace)
        : d(desc), plan(pl), s(sc), P(params), G(grads), fingerprint(fp), image(img), ix(desc),
          c{static_cast<hipStream_t>(stream), static_cast<char*>(workspace), &pl, &sc}, ce(c), cl(c), B(pl.B), F(pl.F), NH(pl.NH), D(pl.D),
          DFF(pl.DFF), Bk((int)pl.Bg), p_drop(pl.drop ? desc->dropout_p : 0.f), inv_keep(pl.drop ? 1.f / (1.f - p_drop) : 1.f),
          scale(1.0f / sqrtf((float)pl.D)), comb(c.f(pl.combined)), hid(c.f(pl.hid)), fused(c.f(pl.fused) /* == combined under torch.cat fusion */),
          h(c.f(pl.h)), hb(c.f(pl.hb)), h2(c.f(pl.h2)), h3(c.f(pl.h3)) {
        if (!grads || pl.inference) return;
        dh3 = c.f(pl.dh3); dh2 = c.f(pl.dh2); dhb = c.f(pl.dhb); dh = c.f(pl.dh); dfused = c.f(pl.dfused); dcomb = c.f(pl.dcomb);
        dlogit = c.f(pl.dlogit); dpre = c.f(pl.dpre);
    }

    // the chain stream (and, `leaves`, the leaf stream) start after the caller's prior work
    int fork(bool leaves) {
        if (!s.overlap) return BBBP_OK;
        TRY(get_side(&ss));
        TRY(fork_side(c.st, ss));
        ce.st = ss->s; ce.side = 1;
        if (leaves) { TRY(after(ss, c.st, ss->leaf)); cl.st = ss->leaf; cl.side = 2; }
        return BBBP_OK;
    }
    // parameter tensor k of encoder layer l, and its gradient
    const float* PL(int l, int k) const { return P[ix.layer(l, k)]; }
    float* GL(int l, int k) const { return G[ix.layer(l, k)]; }
    // the fields that the four per-layer argument tables of the fused encoder schedules (row / sliced, forward / backward) share
    template <typename A> void fill_layer(A& a, int l) const {
        const LayerOff& o = plan.layer[l];
        a.wo = PL(l, L_OUTW); a.g1 = PL(l, L_N1W); a.w1 = PL(l, L_W1); a.w2 = PL(l, L_W2); a.g2 = PL(l, L_N2W);
        a.z1 = c.f(o.z1); a.hff = c.f(o.hff); a.z2 = c.f(o.z2); a.mean1 = c.f(o.mean1); a.rstd1 = c.f(o.rstd1); a.mean2 = c.f(o.mean2); a.rstd2 = c.f(o.rstd2);
        a.seed1 = site_seed(l, 1); a.seed3 = site_seed(l, 3);
    }
    // exact-global-batch mode: the blocks of every rank (forward: (mean, M2); backward: the BatchNorm's two sums, which span every rank's
    // rows) are gathered between the fused head's two launches.  `what`: BBBP_COLL_BN_FWD / BBBP_COLL_BN_BWD
    bbbp_head_sync head_sync(int what) const {
        bbbp_head_sync sync;
        sync.world = plan.world; sync.rank = plan.rank;
        if (plan.exact)
            sync.between = [this, what]() -> int {
                const size_t pcount = (size_t)((B + 15) / 16) * 2 * H1;
                return run_collective(d, BBBP_COLL_ALLGATHER, what, -1, plan.head_partial + (size_t)plan.rank * pcount * sizeof(float), plan.head_partial, pcount, c.st);
            };
        return sync;
    }
    // ---- forward: image branch (R:84-94, 114-115), caller's stream ------------------------------------------------
    int image_fwd() {
        float* pool1 = c.f(plan.pool1); float* pool2 = c.f(plan.pool2);
        {
            Section s1(c.st, SEC_CONV1_FWD);
            TRY(conv3x3_relu_pool_fwd(c.st, image, P[ix.c1_w()], P[ix.c1_b()], pool1, plan.inference ? nullptr : c.u8(plan.mask1), B, 3, C1, IMG, IMG,
                                      c.scratch(), c.scratch_bytes(), s.conv1_fwd));
        }
        {
            Section s2(c.st, SEC_CONV2_FWD);
            TRY(conv3x3_relu_pool_fwd(c.st, pool1, P[ix.c2_w()], P[ix.c2_b()], pool2, plan.inference ? nullptr : c.u8(plan.mask2), B, C1, C2, IMG / 2,
                                      IMG / 2, c.scratch(), c.scratch_bytes(), s.conv2_fwd));
        }
        Section s3(c.st, SEC_IMGFC_FWD);
        (void)bbbp_param_wait(c.st, P[ix.ifc_w()]);        // the optimizer's deferred image-FC slice (bbbp_adamw_step_deferred): first read here
        return linear_fwd(c, pool2, IMG_FLAT, P[ix.ifc_w()], P[ix.ifc_b()], comb + FC, COMB, B, FC, IMG_FLAT, BBBP_ACT_RELU);
    }
    // ---- forward: fingerprint branch = encoder (R:75-78, 110-111) + fingerprint_fc, chain stream; one function per schedule ----
    // the whole chain of a small batch, fingerprint_fc included, as one persistent launch
    int encoder_fwd_sliced() {
        bbbp_enc_sliced_fwd_args a;
        memset(&a, 0, sizeof(a));
        a.x0 = fingerprint; a.L = plan.L; a.B = B; a.F = F; a.DFF = DFF; a.p = p_drop; a.scale = scale;
        a.wfc = P[ix.fpfc_w()]; a.bfc = P[ix.fpfc_b()]; a.comb = comb; a.nfc = FC; a.ldcomb = COMB;
        a.sync = c.u8(plan.sl_sync); a.part = c.f(plan.sl_part);
        for (int l = 0; l < plan.L; ++l) {
            const LayerOff& o = plan.layer[l];
            bbbp_enc_sliced_layer& y = a.lay[l];
            fill_layer(y, l);
            y.win = PL(l, L_INW); y.qkv = c.f(o.qkv); y.prob = c.f(o.prob); y.pd = c.f(o.pd); y.seed0 = site_seed(l, 0);
            y.bin = PL(l, L_INB); y.bo = PL(l, L_OUTB); y.be1 = PL(l, L_N1B); y.b1 = PL(l, L_B1); y.b2 = PL(l, L_B2); y.be2 = PL(l, L_N2B);
            y.ctx = c.f(o.ctx); y.y1 = c.f(o.y1); y.y2 = c.f(o.y2); y.seed2 = site_seed(l, 2);
        }
        return bbbp_enc_sliced_fwd(ce.st, &a);
    }
    // attention launch-per-op, the row-local rest of a layer as one launch
    int encoder_fwd_rows() {
        const float* x = fingerprint;
        // in_proj of layer 0; every later in_proj (and fingerprint_fc) is the tail of the previous layer's row kernel
        TRY(linear_fwd(ce, x, F, PL(0, L_INW), PL(0, L_INB), c.f(plan.layer[0].qkv), 3 * F, B, 3 * F, F, 0));
        for (int l = 0; l < plan.L; ++l) {
            const LayerOff& o = plan.layer[l];
            TRY(attention_fwd_gemm(l, x));
            bbbp_enc_row_fwd_args a;
            fill_layer(a, l);
            a.ctx = c.f(o.ctx); a.xin = x;
            a.bo = PL(l, L_OUTB); a.be1 = PL(l, L_N1B); a.b1 = PL(l, L_B1); a.b2 = PL(l, L_B2); a.be2 = PL(l, L_N2B);
            const bool last = l + 1 == plan.L;
            a.wn = last ? P[ix.fpfc_w()] : PL(l + 1, L_INW); a.bn = last ? P[ix.fpfc_b()] : PL(l + 1, L_INB);
            a.outn = last ? comb : c.f(plan.layer[l + 1].qkv); a.nn = last ? FC : 3 * F; a.ldn = last ? COMB : 3 * F; a.actn = last ? 1 : 0;
            a.y1 = c.f(o.y1); a.y2 = c.f(o.y2);
            a.B = B; a.F = F; a.DFF = DFF; a.p = p_drop; a.seed2 = site_seed(l, 2);
            TRY(bbbp_enc_row_fwd(ce.st, &a));
            x = c.f(o.y2);
        }
        return BBBP_OK;
    }
    int encoder_fwd_ops() {
        if (plan.fold) {
            // W' = Wo Wv, b' = Wo bv of every layer in one launch at the head of the chain (the parameters change every step)
            const float* win[32]; const float* bin[32]; const float* wo[32]; const float* bo[32]; float* wf[32]; float* bf[32]; float* wvt[32];
            for (int l = 0; l < plan.L; ++l) {
                win[l] = PL(l, L_INW); bin[l] = PL(l, L_INB); wo[l] = PL(l, L_OUTW);
                // fused attention (forward-only, no dropout): softmax rows sum to one, so out_proj's bias is carried by b' = Wo bv + bo
                bo[l] = plan.attn_b3 ? PL(l, L_OUTB) : nullptr;
                wf[l] = c.f(plan.fwf[l]); bf[l] = c.f(plan.fbf[l]); wvt[l] = c.f(plan.fwvt[l]);
            }
            TRY(bbbp_outproj_fold(ce.st, plan.L, F, win, bin, wo, bo, wf, bf, wvt));
        }
        const float* x = fingerprint;
        PendingNorm pend;
        for (int l = 0; l < plan.L; ++l) TRY(encoder_layer_fwd_ops(l, x, pend));
        return fingerprint_fc_fwd(x, pend);
    }
    // x = LayerNorm(pend.z) (written to pend.y) where a norm2 is pending; y = act(x W^T + b) in the same launch then
    int linear_after_norm(PendingNorm& pend, const float* x, const float* W, const float* b, float* y, int ldy, int N, int act) {
        if (!pend.z) return linear_fwd(ce, x, F, W, b, y, ldy, B, N, F, act);
        const float* z = pend.z;
        pend.z = nullptr;
        return bbbp_layernorm_linear_fwd(ce.st, z, F, pend.gamma, pend.beta, 1e-5f, W, b, y, ldy, act, 0.f, 0, pend.y, F, pend.mean, pend.rstd, B, N, F);
    }
    // fingerprint_fc (R:79-82, 112) -> combined[:, 0:128]
    int fingerprint_fc_fwd(const float* x, PendingNorm& pend) { return linear_after_norm(pend, x, P[ix.fpfc_w()], P[ix.fpfc_b()], comb, COMB, FC, BBBP_ACT_RELU); }
    // scores -> softmax (+ dropout) -> context with materialised probabilities: into ctx, or (folded plan, one head) z1 = Pd VW + bo
    // (the row-fused schedule's attention too: never folded, absorbed or exact there)
    int attention_fwd_gemm(int l, const float* x) {
        const LayerOff& o = plan.layer[l];
        float* qkv = c.f(o.qkv); float* prob = c.f(o.prob);
        // keys and values: this rank's rows of qkv, or (exact-global-batch mode) the rows of every rank, gathered once per layer
        const float* kmat = qkv + F; const float* vmat = qkv + 2 * F; int ldkv = 3 * F;
        if (plan.exact) {
            float* kvg = c.f(o.kvg);
            const long n = (long)B * 2 * F;
            hipLaunchKernelGGL(kv_pack_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), g_bbbp_small_lds_pad, ce.st, qkv, kvg + (size_t)plan.rank * n, n, F);
            BBBP_CHECK_LAUNCH();
            TRY(run_collective(d, BBBP_COLL_ALLGATHER, BBBP_COLL_KV, l, o.kvg + (size_t)plan.rank * n * sizeof(float), o.kvg, (size_t)n, ce.st));
            kmat = kvg; vmat = kvg + F; ldkv = 2 * F;
        }
        // scores_h = scale * Q_h K_h^T
        TRY(bbbp_gemm_f32(ce.st, 0, 1, B, Bk, D, scale, qkv, 3 * F, kmat, ldkv, prob, Bk, nullptr, nullptr, 0, 0, NH, D, D,
                          (long)B * Bk, 0, ce.scratch(), ce.scratch_bytes()));
        float* pd = c.f(o.pd);
        TRY(bbbp_softmax_fwd(ce.st, prob, pd, (long)NH * B, Bk, p_drop, site_seed(l, 0)));
        // ctx_h = Pd_h V_h; folded plan (one head): z1 = Pd VW + bo, the out_proj output itself
        if (!(plan.fold && s.absorb1))
            return bbbp_gemm_f32(ce.st, 0, 0, B, D, Bk, 1.f, pd, Bk, vmat, ldkv, plan.fold ? c.f(o.z1) : c.f(o.ctx), F, plan.fold ? PL(l, L_OUTB) : nullptr,
                                 nullptr, 0, 0, NH, (long)B * Bk, D, D, 0, ce.scratch(), ce.scratch_bytes());
        // ... and with norm1 absorbed by linear1, z1 = dropout(Pd VW + bo) + x: what bbbp_layernorm_fwd would have left in z1
        bbbp_gemm_desc g = gemm_desc(0, 0, B, D, Bk, 1.f, pd, Bk, vmat, ldkv, c.f(o.z1), F, 1, 0, 0, 0);
        g.bias = PL(l, L_OUTB); g.residual = x; g.ldr = F; g.drop_p = p_drop; g.drop_seed = site_seed(l, 1);
        return bbbp_gemm_f32_grouped(ce.st, &g, 1, ce.scratch(), ce.scratch_bytes());
    }
    // one layer of the launch-per-op schedule; x: the layer's input on entry, its output on return.
    // LayerNorm absorbed by the Linear that consumes it (s.absorb1 / s.absorb2; gemm.hip: gemm_direct_lna_kernel): norm1 -> linear1, norm2 ->
    // the next in_proj / fingerprint_fc.  The dropout + residual that the LayerNorm launch applied to its input move into the epilogue of the
    // GEMM that produces it (same Philox elements), so z1 / z2, y1 / y2 and the row statistics the backward pass reads are the same tensors.
    int encoder_layer_fwd_ops(int l, const float*& x, PendingNorm& pend) {
        const LayerOff& o = plan.layer[l];
        float* qkv = c.f(o.qkv); float* ctx = c.f(o.ctx);
        {
            Section sq(ce.st, SEC_QKV_FWD);
            // folded plan: [Q | K | VW] = x [Wq; Wk; Wo Wv]^T + [bq; bk; Wo bv]; the previous layer's absorbed norm2 is applied by the same launch
            TRY(linear_after_norm(pend, x, plan.fold ? c.f(plan.fwf[l]) : PL(l, L_INW), plan.fold ? c.f(plan.fbf[l]) : PL(l, L_INB), qkv, 3 * F, 3 * F, 0));
        }
        {
            Section sec_attn(ce.st, SEC_ATTN_FWD);
            if (plan.attn_b3) {
                TRY(bbbp_attn_b3_fwd(ce.st, qkv, plan.fold ? c.f(o.z1) : ctx, B, F, NH, scale, plan.attn_part_bytes ? c.f(plan.attn_part) : nullptr, plan.attn_part_bytes));
            } else if (plan.flash) {
                TRY(bbbp_attn_small_fwd(ce.st, qkv, ctx, c.f(o.lse), B, F, NH, scale, p_drop, site_seed(l, 0), o.keep ? c.u8(o.keep) : nullptr));
            } else {
                TRY(attention_fwd_gemm(l, x));
            }
        }
        float* z1 = c.f(o.z1); float* y1 = c.f(o.y1);
        if (s.ln_fused) {
            // out_proj -> (dropout) + residual -> norm1: one launch when the output is narrow (gemm.hip: gemm_direct_ln_kernel)
            TRY(bbbp_linear_layernorm_fwd(ce.st, ctx, F, PL(l, L_OUTW), PL(l, L_OUTB), x, F, z1, F, y1, F, PL(l, L_N1W),
                                          PL(l, L_N1B), c.f(o.mean1), c.f(o.rstd1), B, F, F, 1e-5f, p_drop, site_seed(l, 1)));
        } else {
            if (!plan.fold) {
                Section so(ce.st, SEC_OUTPROJ_FWD);
                if (s.absorb1) {
                    bbbp_gemm_desc g = gemm_desc(0, 1, B, F, F, 1.f, ctx, F, PL(l, L_OUTW), F, z1, F, 1, 0, 0, 0);
                    g.bias = PL(l, L_OUTB); g.residual = x; g.ldr = F; g.drop_p = p_drop; g.drop_seed = site_seed(l, 1);
                    TRY(bbbp_gemm_f32_grouped(ce.st, &g, 1, ce.scratch(), ce.scratch_bytes()));
                } else {
                    TRY(linear_fwd(ce, ctx, F, PL(l, L_OUTW), PL(l, L_OUTB), z1, F, B, F, F, 0));
                }
            }
            if (!s.absorb1) {
                Section sl(ce.st, SEC_LN_FWD);
                TRY(bbbp_layernorm_fwd(ce.st, z1, x, y1, PL(l, L_N1W), PL(l, L_N1B), c.f(o.mean1), c.f(o.rstd1), B, F, 1e-5f, p_drop, site_seed(l, 1)));
            }
        }
        float* hff = c.f(o.hff); float* z2 = c.f(o.z2); float* y2 = c.f(o.y2);
        // linear1 + ReLU (+ the FFN dropout in the same epilogue when the product takes the small-GEMM path: same Philox elements as bbbp_dropout)
        {
            Section sf(ce.st, SEC_FFN1_FWD);
            if (s.absorb1) {
                // norm1 absorbed: hff = dropout(ReLU(LayerNorm(z1) W1^T + b1)); y1, mean1, rstd1 written by the same launch
                TRY(bbbp_layernorm_linear_fwd(ce.st, z1, F, PL(l, L_N1W), PL(l, L_N1B), 1e-5f, PL(l, L_W1), PL(l, L_B1),
                                              hff, DFF, BBBP_ACT_RELU, p_drop, site_seed(l, 2), y1, F, c.f(o.mean1), c.f(o.rstd1), B, DFF, F));
            } else if (s.drop_in_gemm) {
                bbbp_gemm_desc g = gemm_desc(0, 1, B, DFF, F, 1.f, y1, F, PL(l, L_W1), F, hff, DFF, 1, 0, 0, 0);
                g.bias = PL(l, L_B1); g.act = BBBP_ACT_RELU; g.drop_p = p_drop; g.drop_seed = site_seed(l, 2);
                TRY(bbbp_gemm_f32_grouped(ce.st, &g, 1, ce.scratch(), ce.scratch_bytes()));
            } else {
                TRY(linear_fwd(ce, y1, F, PL(l, L_W1), PL(l, L_B1), hff, DFF, B, DFF, F, BBBP_ACT_RELU));
            }
        }
        if (plan.drop && !s.drop_in_gemm && !s.absorb1) TRY(bbbp_dropout(ce.st, hff, hff, (long)B * DFF, p_drop, site_seed(l, 2)));
        {
            Section sf(ce.st, SEC_FFN2_FWD);
            if (s.absorb2) {
                // norm2 is absorbed by the next in_proj (or fingerprint_fc): z2 = dropout(h W2^T + b2) + y1 here, normalised there
                bbbp_gemm_desc g = gemm_desc(0, 1, B, F, DFF, 1.f, hff, DFF, PL(l, L_W2), DFF, z2, F, 1, 0, 0, 0);
                g.bias = PL(l, L_B2); g.residual = y1; g.ldr = F; g.drop_p = p_drop; g.drop_seed = site_seed(l, 3);
                TRY(bbbp_gemm_f32_grouped(ce.st, &g, 1, ce.scratch(), ce.scratch_bytes()));
                pend.z = z2; pend.gamma = PL(l, L_N2W); pend.beta = PL(l, L_N2B); pend.y = y2; pend.mean = c.f(o.mean2); pend.rstd = c.f(o.rstd2);
            } else {
                TRY(linear_fwd(ce, hff, DFF, PL(l, L_W2), PL(l, L_B2), z2, F, B, F, DFF, 0));
            }
        }
        if (!s.absorb2) {
            Section sl(ce.st, SEC_LN_FWD);
            TRY(bbbp_layernorm_fwd(ce.st, z2, y1, y2, PL(l, L_N2W), PL(l, L_N2B), c.f(o.mean2), c.f(o.rstd2), B, F, 1e-5f, p_drop, site_seed(l, 3)));
        }
        x = y2;
        return BBBP_OK;
    }
    // ---- forward: fusion block (R:60-65, 117) + regression head (R:98-107, 118), caller's stream ----------------------
    // two launches (head.hip); with torch.cat fusion the first launch starts at fc.0
    int head_fwd_fused(float* const* bn_running, float* out) {
        const float *fw1[4] = {}, *fb1[4] = {}, *fw2[4] = {}, *fb2[4] = {};
        if (!plan.concat)
            for (int hh = 0; hh < 4; ++hh) { fw1[hh] = P[ix.fus(hh, 0)]; fb1[hh] = P[ix.fus(hh, 1)]; fw2[hh] = P[ix.fus(hh, 2)]; fb2[hh] = P[ix.fus(hh, 3)]; }
        const bbbp_head_sync sync = head_sync(BBBP_COLL_BN_FWD);
        return bbbp_head_forward_fused_sync(c.st, comb, fw1, fb1, fw2, fb2, P[ix.fc0_w()], P[ix.fc0_b()], P[ix.bn_w()], P[ix.bn_b()],
                                            bn_running[0], bn_running[1], P[ix.fc3_w()], P[ix.fc3_b()], P[ix.fc5_w()], P[ix.fc5_b()],
                                            P[ix.fc7_w()], P[ix.fc7_b()], hid, c.f(plan.attn), fused, h, hb, c.f(plan.bn_mean), c.f(plan.bn_rstd), h2, h3, out,
                                            c.f(plan.head_partial), B, d->training, plan.concat ? 1 : 0, plan.exact ? &sync : nullptr);
    }
    int head_fwd_ops(float* const* bn_running, float* out) {
        if (!plan.concat) {
            const float* w2[NHEADS_FUSION]; const float* b2[NHEADS_FUSION];
            for (int hh = 0; hh < NHEADS_FUSION; ++hh) {
                TRY(linear_fwd(c, comb, COMB, P[ix.fus(hh, 0)], P[ix.fus(hh, 1)], hid + (size_t)hh * B * FUS_HID, FUS_HID, B, FUS_HID, COMB, BBBP_ACT_TANH));
                w2[hh] = P[ix.fus(hh, 2)]; b2[hh] = P[ix.fus(hh, 3)];
            }
            TRY(bbbp_fusion_combine_fwd(c.st, comb, hid, w2, b2, fused, c.f(plan.attn), B, COMB, FUS_HID, NHEADS_FUSION));
        }
        TRY(linear_fwd(c, fused, COMB, P[ix.fc0_w()], P[ix.fc0_b()], h, H1, B, H1, COMB, BBBP_ACT_RELU));
        TRY(bbbp_batchnorm1d_fwd(c.st, h, hb, P[ix.bn_w()], P[ix.bn_b()], bn_running[0], bn_running[1], c.f(plan.bn_mean),
                                 c.f(plan.bn_rstd), B, H1, 1e-5f, 0.1f, d->training));
        TRY(linear_fwd(c, hb, H1, P[ix.fc3_w()], P[ix.fc3_b()], h2, H2, B, H2, H1, BBBP_ACT_RELU));
        TRY(linear_fwd(c, h2, H2, P[ix.fc5_w()], P[ix.fc5_b()], h3, H3, B, H3, H2, BBBP_ACT_RELU));
        return linear_fwd(c, h3, H3, P[ix.fc7_w()], P[ix.fc7_b()], out, 1, B, 1, H3, 0);
    }
    // ---- backward: leaves (leaf stream) -----------------------------------------------------------------------------
    int leaf_after(const Ctx& producer) { return ss ? after(ss, producer.st, cl.st) : BBBP_OK; }
    // The head's weight / bias gradients in leaf-stream order: 0..3 fc.7, fc.5, fc.3, fc.0; 4 + h fusion head h; 8 the image FC's bias (column
    // sums of the masked dcomb).  The fused head enqueues them all after the image branch; the launch-per-op head one by one as its chain
    // writes what they read.
    int head_leaf(int k, const float* dout) {
        switch (k) {
        case 0: return linear_bwd_weight_bias(cl, dout, 1, h3, H3, G[ix.fc7_w()], G[ix.fc7_b()], B, 1, H3);
        case 1: return linear_bwd_weight_bias(cl, dh3, H3, h2, H2, G[ix.fc5_w()], G[ix.fc5_b()], B, H3, H2);
        case 2: return linear_bwd_weight_bias(cl, dh2, H2, hb, H1, G[ix.fc3_w()], G[ix.fc3_b()], B, H2, H1);
        case 3: return linear_bwd_weight_bias(cl, dh, H1, fused, COMB, G[ix.fc0_w()], G[ix.fc0_b()], B, H1, COMB);
        case 8: return bbbp_bias_act_bwd(cl.st, dcomb + FC, COMB, nullptr, 0, G[ix.ifc_b()], B, FC, 0, 1.f);
        }
        if (plan.concat) return BBBP_OK;
        const int hh = k - 4;
        float* dp = dpre + (size_t)hh * B * FUS_HID;
        TRY(linear_bwd_weight_bias(cl, dlogit + (size_t)hh * B, 1, hid + (size_t)hh * B * FUS_HID, FUS_HID, G[ix.fus(hh, 2)], G[ix.fus(hh, 3)], B, 1, FUS_HID));
        return linear_bwd_weight_bias(cl, dp, FUS_HID, comb, COMB, G[ix.fus(hh, 0)], G[ix.fus(hh, 1)], B, FUS_HID, COMB);
    }
    int head_leaves(const float* dout) { for (int k = 0; k <= 8; ++k) TRY(head_leaf(k, dout)); return BBBP_OK; }
    // A layer's weight / bias gradients: linear2 and linear1, out_proj, in_proj (the schedules put chain work between them); `timed`: the
    // launch-per-op schedule's profiling sections
    int ffn_leaves(int l, bool timed) {
        const LayerOff& o = plan.layer[l]; const LayerGrad& g = plan.lgrad[l];
        {
            Section sw(cl.st, timed ? SEC_FFN2_WGRAD : -1);
            TRY(linear_bwd_weight_bias(cl, c.f(g.dz2d), F, c.f(o.hff), DFF, GL(l, L_W2), GL(l, L_B2), B, F, DFF));
        }
        Section sw(cl.st, timed ? SEC_FFN1_WGRAD : -1);
        return linear_bwd_weight_bias(cl, c.f(g.dhff), DFF, c.f(o.y1), F, GL(l, L_W1), GL(l, L_B1), B, DFF, F);
    }
    int outproj_leaf(int l, bool timed) {
        Section sw(cl.st, timed ? SEC_OUTPROJ_WGRAD : -1);
        return linear_bwd_weight_bias(cl, c.f(plan.lgrad[l].dz1d), F, c.f(plan.layer[l].ctx), F, GL(l, L_OUTW), GL(l, L_OUTB), B, F, F);
    }
    int inproj_leaf(int l, bool timed) {
        Section sw(cl.st, timed ? SEC_QKV_WGRAD : -1);
        return linear_bwd_weight_bias(cl, c.f(plan.lgrad[l].dqkv), 3 * F, layer_input(l), F, GL(l, L_INW), GL(l, L_INB), B, 3 * F, F);
    }
    const float* layer_input(int l) const { return l > 0 ? c.f(plan.layer[l - 1].y2) : fingerprint; }      // l == L: the encoder's output
    int fingerprint_fc_leaf() { return linear_bwd_weight_bias(cl, dcomb, COMB, layer_input(plan.L), F, G[ix.fpfc_w()], G[ix.fpfc_b()], B, FC, F); }
    // both LayerNorms' weight / bias gradients of layer l in ONE leaf launch (dgamma = sum_rows dy * xhat, dbeta = sum_rows dy),
    // the last leaf of the layer: its gradient bucket (all twelve tensors, one contiguous slice) is final after it
    int layer_norm_grads(int l) {
        const LayerOff& o = plan.layer[l]; const LayerGrad& g = plan.lgrad[l];
        const float* dy[2] = {c.f(g.dyout), c.f(g.dy1)}; const float* zz[2] = {c.f(o.z2), c.f(o.z1)};
        const float* mm[2] = {c.f(o.mean2), c.f(o.mean1)}; const float* rr[2] = {c.f(o.rstd2), c.f(o.rstd1)};
        float* dg[2] = {GL(l, L_N2W), GL(l, L_N1W)}; float* db[2] = {GL(l, L_N2B), GL(l, L_N1B)};
        return bbbp_ln_param_grad_multi(cl.st, 2, dy, zz, mm, rr, dg, db, B, F);
    }
    int record_layer_bucket(int l) { return (ds && l >= 0 && l < 32) ? record_bucket(ds->layer[l], cl.st) : BBBP_OK; }
    int layer_norm_leaves(int l) { TRY(layer_norm_grads(l)); return record_layer_bucket(l); }
    // ---- backward: head and fusion block (chain on the caller's stream) ----------------------------------------------
    // the whole input-gradient chain of the head and the fusion block in two launches (head.hip); every weight / bias
    // gradient is a leaf that reads what those wrote
    int head_bwd_fused(const float* dout) {
        const float* fw1[NHEADS_FUSION]; const float* fw2[NHEADS_FUSION];
        for (int hh = 0; hh < NHEADS_FUSION; ++hh) { fw1[hh] = P[ix.fus(hh, 0)]; fw2[hh] = P[ix.fus(hh, 2)]; }
        const bbbp_head_sync sync = head_sync(BBBP_COLL_BN_BWD);
        TRY(bbbp_head_backward_fused_sync(c.st, dout, comb, hid, c.f(plan.attn), h, h2, h3, c.f(plan.bn_mean), c.f(plan.bn_rstd),
                                          P[ix.bn_w()], fw1, fw2, P[ix.fc0_w()], P[ix.fc3_w()], P[ix.fc5_w()], P[ix.fc7_w()], dh3, dh2, dhb,
                                          dh, dlogit, dpre, dcomb, G[ix.bn_w()], G[ix.bn_b()], c.f(plan.head_partial), B, d->training,
                                          plan.exact ? &sync : nullptr));
        return leaf_after(c);          // (the leaves themselves: after the image branch's kernels, the host reaches those sooner)
    }
    // dx = (dy W) (.) [gate > 0] on the caller's stream: the ReLU masks ride in the input-gradient GEMMs' epilogues
    int gated_bwd_input(const float* dy, int N, const float* W, float* dx, int K, const float* gate) {
        bbbp_gemm_desc g = gemm_desc(0, 0, B, K, N, 1.f, dy, N, W, K, dx, K);
        g.gate = gate; g.ldg = K;
        return bbbp_gemm_f32_grouped(c.st, &g, 1, c.scratch(), c.scratch_bytes());
    }
    int head_bwd_ops(const float* dout) {
        // fc.7: out = h3 W7^T + b7
        TRY(head_leaf(0, dout));
        TRY(gated_bwd_input(dout, 1, P[ix.fc7_w()], dh3, H3, h3));
        TRY(leaf_after(c));
        TRY(head_leaf(1, dout));
        TRY(gated_bwd_input(dh3, H3, P[ix.fc5_w()], dh2, H2, h2));
        TRY(leaf_after(c));
        TRY(head_leaf(2, dout));
        TRY(linear_bwd_input(c, dh2, H2, P[ix.fc3_w()], dhb, H1, B, H2, H1));
        TRY(bbbp_batchnorm1d_bwd_relu(c.st, dhb, h, P[ix.bn_w()], c.f(plan.bn_mean), c.f(plan.bn_rstd), dh, G[ix.bn_w()], G[ix.bn_b()], B, H1, d->training));
        TRY(leaf_after(c));
        TRY(head_leaf(3, dout));
        if (plan.concat) {
            // torch.cat fusion: dcomb = dh W0, masked by the ReLUs that produced combined = [fp_out | img_out]
            TRY(gated_bwd_input(dh, H1, P[ix.fc0_w()], dcomb, COMB, comb));
        } else {
            TRY(linear_bwd_input(c, dh, H1, P[ix.fc0_w()], dfused, COMB, B, H1, COMB));
            // attention fusion
            const float* w2[NHEADS_FUSION];
            for (int hh = 0; hh < NHEADS_FUSION; ++hh) w2[hh] = P[ix.fus(hh, 2)];
            TRY(bbbp_fusion_combine_bwd(c.st, dfused, comb, hid, c.f(plan.attn), w2, dcomb, dlogit, dpre, B, COMB, FUS_HID, NHEADS_FUSION));
            TRY(leaf_after(c));
            for (int hh = 0; hh < NHEADS_FUSION; ++hh) {
                TRY(head_leaf(4 + hh, dout));
                // dcomb += dp W1_h; the last of the four also applies the ReLU mask of both branch outputs (combined = [fp_out | img_out])
                bbbp_gemm_desc g = gemm_desc(0, 0, B, COMB, FUS_HID, 1.f, dpre + (size_t)hh * B * FUS_HID, FUS_HID, P[ix.fus(hh, 0)], COMB, dcomb, COMB);
                g.residual = dcomb; g.ldr = COMB;
                if (hh == NHEADS_FUSION - 1) { g.gate = comb; g.ldg = COMB; g.gate_after_residual = 1; }
                TRY(bbbp_gemm_f32_grouped(c.st, &g, 1, c.scratch(), c.scratch_bytes()));
            }
        }
        // bias gradients of the two branch outputs: leaves of the masked dcomb
        TRY(leaf_after(c));
        return head_leaf(8, dout);
    }
    // ---- backward: image branch (caller's stream), five long MFMA-bound kernels; `sec`: the open section of that stream ----
    int image_bwd(std::optional<Section>& sec) {
        auto next_section = [&](int id) { sec.reset(); sec.emplace(c.st, id); };
        float* pool1 = c.f(plan.pool1); float* pool2 = c.f(plan.pool2);
        float* dpool2 = c.f(plan.dpool2); float* dpool1 = c.f(plan.dpool1);
        next_section(SEC_IMGFC_BWD);
        TRY(linear_bwd_weight(c, dcomb + FC, COMB, pool2, IMG_FLAT, G[ix.ifc_w()], B, FC, IMG_FLAT));
        if (ds) TRY(record_bucket(ds->bucket0, c.st));
        TRY(linear_bwd_input(c, dcomb + FC, COMB, P[ix.ifc_w()], dpool2, IMG_FLAT, B, FC, IMG_FLAT));
        if (ds) {
            // ... and from here on the image-FC weight itself is no longer read by this pass (bbbp_mixed_backward_wait_released, bucket 0)
            BucketEvent& rel = ds->bucket0_released;
            rel.recorded = g_release_events && ds->bucket0.recorded;
            if (rel.recorded) {
                if (!rel.ev) BBBP_CHECK_HIP(hipEventCreateWithFlags(&rel.ev, hipEventDisableTiming));
                BBBP_CHECK_HIP(hipEventRecord(rel.ev, c.st));
            }
        }
        next_section(SEC_CONV2_WGRAD);
        TRY(conv3x3_relu_pool_bwd_weight(c.st, pool1, dpool2, c.u8(plan.mask2), G[ix.c2_w()], G[ix.c2_b()], B, C1, C2, IMG / 2, IMG / 2,
                                         c.scratch(), c.scratch_bytes(), s.conv2_wgrad));
        next_section(SEC_CONV2_DGRAD);
        TRY(bbbp_conv3x3_relu_pool_bwd_data(c.st, dpool2, c.u8(plan.mask2), P[ix.c2_w()], dpool1, B, C1, C2, IMG / 2, IMG / 2, c.scratch(), c.scratch_bytes()));
        next_section(SEC_CONV1_WGRAD);
        TRY(bbbp_conv3x3_relu_pool_bwd_weight(c.st, image, dpool1, c.u8(plan.mask1), G[ix.c1_w()], G[ix.c1_b()], B, 3, C1, IMG, IMG, c.scratch(), c.scratch_bytes()));
        sec.reset();
        return BBBP_OK;
    }
    // ---- backward: fingerprint branch, chain on `ce`, leaves on `cl`; one function per schedule ------------------------
    // gradient of the encoder's output (of the fingerprint, on request, when there are no layers)
    int fingerprint_fc_bwd_input() {
        if (plan.L == 0 && !d->need_input_grad) return BBBP_OK;
        return linear_bwd_input(ce, dcomb, COMB, P[ix.fpfc_w()], plan.L > 0 ? c.f(plan.lgrad[plan.L - 1].dyout) : c.f(plan.dA), F, B, FC, F);
    }
    // in_proj input gradient of layer 0 of the fused schedules, on request
    int fingerprint_grad_fused() {
        if (!d->need_input_grad) return BBBP_OK;
        return linear_bwd_input(ce, c.f(plan.lgrad[0].dqkv), 3 * F, PL(0, L_INW), c.f(plan.dA), F, B, 3 * F, F, c.f(plan.lgrad[0].dz1), F);
    }
    // the whole input-gradient chain (fingerprint_fc's included) in one persistent launch; every weight gradient is a leaf of its buffers afterwards
    int encoder_bwd_sliced() {
        bbbp_enc_sliced_bwd_args a;
        memset(&a, 0, sizeof(a));
        a.dcomb = dcomb; a.ldcomb = COMB; a.nfc = FC; a.wfc = P[ix.fpfc_w()];
        a.L = plan.L; a.B = B; a.F = F; a.DFF = DFF; a.p = p_drop; a.scale = scale;
        a.sync = c.u8(plan.sl_sync); a.part = c.f(plan.sl_part); a.kvpart = c.f(plan.sl_kvpart);
        for (int l = 0; l < plan.L; ++l) {
            const LayerOff& o = plan.layer[l]; const LayerGrad& g = plan.lgrad[l];
            bbbp_enc_sliced_bwd_layer& y = a.lay[l];
            fill_layer(y, l);
            y.win = PL(l, L_INW); y.qkv = c.f(o.qkv); y.prob = c.f(o.prob); y.pd = c.f(o.pd); y.seed0 = site_seed(l, 0);
            y.dyout = c.f(g.dyout); y.dz2 = c.f(g.dz2); y.dff = c.f(g.dz2d); y.dhff = c.f(g.dhff); y.dy1 = c.f(g.dy1);
            y.dz1 = c.f(g.dz1); y.dsa = c.f(g.dz1d); y.dqkv = c.f(g.dqkv);
        }
        TRY(bbbp_enc_sliced_bwd(ce.st, &a));
        TRY(fingerprint_grad_fused());
        TRY(leaf_after(ce));
        for (int l = plan.L - 1; l >= 0; --l) {
            TRY(ffn_leaves(l, false));
            TRY(outproj_leaf(l, false));
            TRY(inproj_leaf(l, false));
            TRY(layer_norm_leaves(l));
        }
        return BBBP_OK;
    }
    int encoder_bwd_rows() {
        TRY(fingerprint_fc_bwd_input());
        float* dctx = c.f(plan.dctx);
        for (int l = plan.L - 1; l >= 0; --l) {
            const LayerGrad& g = plan.lgrad[l];
            // one launch: (in_proj input gradient of the layer above + residual ->) norm2 bwd -> linear2 dgrad (.) gate -> linear1
            // dgrad + residual -> norm1 bwd -> out_proj dgrad
            bbbp_enc_row_bwd_args a;
            fill_layer(a, l);
            const bool top = l + 1 == plan.L;
            a.dqkv_up = top ? nullptr : c.f(plan.lgrad[l + 1].dqkv); a.win_up = top ? nullptr : PL(l + 1, L_INW);
            a.dz1_up = top ? nullptr : c.f(plan.lgrad[l + 1].dz1); a.dyout = c.f(g.dyout);
            a.dz2 = c.f(g.dz2); a.dff = c.f(g.dz2d); a.dhff = c.f(g.dhff); a.dy1 = c.f(g.dy1); a.dz1 = c.f(g.dz1); a.dsa = c.f(g.dz1d); a.dctx = dctx;
            a.B = B; a.F = F; a.DFF = DFF; a.p = p_drop;
            TRY(bbbp_enc_row_bwd(ce.st, &a));
            TRY(leaf_after(ce));
            TRY(ffn_leaves(l, false));
            TRY(outproj_leaf(l, false));
            TRY(attention_bwd_gemm(l, dctx));
            TRY(leaf_after(ce));
            TRY(inproj_leaf(l, false));
            TRY(layer_norm_leaves(l));
        }
        return fingerprint_grad_fused();
    }
    int encoder_bwd_ops() { TRY(fingerprint_fc_bwd_input()); for (int l = plan.L - 1; l >= 0; --l) TRY(encoder_layer_bwd_ops(l)); return BBBP_OK; }
    // attention backward with materialised probabilities (both launch-per-op and row-fused schedules).  Products that become ready together share a launch (bbbp_gemm_f32_grouped):
    //   dV_h = Pd_h^T dctx_h -> dqkv[:, 2F + hD]   |   dPd_h = dctx_h V_h^T
    int attention_bwd_gemm(int l, const float* dattn) {
        const LayerOff& o = plan.layer[l];
        float* qkv = c.f(o.qkv); float* dqkv = c.f(plan.lgrad[l].dqkv); float* dprob = c.f(plan.dprob);
        // exact-global-batch mode: keys / values are the gathered rows of every rank; dK | dV of ALL keys (this rank's queries' share)
        // go to dkvg and come back reduce-scattered
        const float* kmat = plan.exact ? c.f(o.kvg) : qkv + F; const float* vmat = plan.exact ? c.f(o.kvg) + F : qkv + 2 * F;
        const int ldkv = plan.exact ? 2 * F : 3 * F;
        float* dkmat = plan.exact ? c.f(plan.dkvg) : dqkv + F; float* dvmat = plan.exact ? c.f(plan.dkvg) + F : dqkv + 2 * F;
        {
            bbbp_gemm_desc g[2] = {
                gemm_desc(1, 0, Bk, D, B, 1.f, c.f(o.pd), Bk, dattn, F, dvmat, ldkv, NH, (long)B * Bk, D, D),
                gemm_desc(0, 1, B, Bk, D, 1.f, dattn, F, vmat, ldkv, dprob, Bk, NH, D, D, (long)B * Bk)};
            TRY(bbbp_gemm_f32_grouped(ce.st, g, 2, ce.scratch(), ce.scratch_bytes()));
        }
        TRY(bbbp_softmax_bwd(ce.st, dprob, c.f(o.prob), (long)NH * B, Bk, p_drop, site_seed(l, 0)));
        //   dQ_h = scale dS_h K_h   |   dK_h = scale dS_h^T Q_h
        {
            bbbp_gemm_desc g[2] = {
                gemm_desc(0, 0, B, D, Bk, scale, dprob, Bk, kmat, ldkv, dqkv, 3 * F, NH, (long)B * Bk, D, D),
                gemm_desc(1, 0, Bk, D, B, scale, dprob, Bk, qkv, 3 * F, dkmat, ldkv, NH, (long)B * Bk, D, D)};
            TRY(bbbp_gemm_f32_grouped(ce.st, g, 2, ce.scratch(), ce.scratch_bytes()));
        }
        if (plan.exact) {
            const long n = (long)B * 2 * F;
            TRY(run_collective(d, BBBP_COLL_REDUCE_SCATTER, BBBP_COLL_DKV, l, plan.dkvg, plan.dkvl, (size_t)n, ce.st));
            hipLaunchKernelGGL(kv_unpack_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), g_bbbp_small_lds_pad, ce.st, c.f(plan.dkvl), dqkv, n, F);
            BBBP_CHECK_LAUNCH();
        }
        return BBBP_OK;
    }
    // folded plan: [dWq; dWk | dbq; dbk] straight into the gradient, the folded block dW' | db' = dVW^T [x | 1] into its scratch (one launch), then
    // dWo = dW' Wv^T + db' bv^T, d[Wv | bv] = Wo^T [dW' | db'] and dbo = column sums of dsa in one more (fold.hip)
    int folded_attn_leaves(int l) {
        Section sw(cl.st, SEC_QKV_WGRAD);
        const float* xin = layer_input(l);
        float* dqkv = c.f(plan.lgrad[l].dqkv); float* tdw = c.f(plan.ftdw[l]); float* tdb = c.f(plan.ftdb[l]);
        if (bbbp_gemm_folds_asum(2 * F, F, B, 1) && bbbp_gemm_folds_asum(F, F, B, 1)) {
            bbbp_gemm_desc gg[2] = {gemm_desc(1, 0, 2 * F, F, B, 1.f, dqkv, 3 * F, xin, F, GL(l, L_INW), F, 1, 0, 0, 0),
                                    gemm_desc(1, 0, F, F, B, 1.f, dqkv + 2 * F, 3 * F, xin, F, tdw, F, 1, 0, 0, 0)};
            gg[0].asum = GL(l, L_INB); gg[1].asum = tdb;
            TRY(bbbp_gemm_f32_grouped(cl.st, gg, 2, cl.scratch(), cl.scratch_bytes()));
        } else {
            TRY(linear_bwd_weight_bias(cl, dqkv, 3 * F, xin, F, GL(l, L_INW), GL(l, L_INB), B, 2 * F, F));
            TRY(linear_bwd_weight_bias(cl, dqkv + 2 * F, 3 * F, xin, F, tdw, tdb, B, F, F));
        }
        return bbbp_outproj_unfold(cl.st, F, B, tdw, tdb, PL(l, L_OUTW), c.f(plan.fwvt[l]), c.f(plan.lgrad[l].dz1d), F, GL(l, L_OUTW),
                                   GL(l, L_OUTB), GL(l, L_INW) + (size_t)2 * F * F, GL(l, L_INB) + 2 * F);
    }
    int encoder_layer_bwd_ops(int l) {
        const LayerOff& o = plan.layer[l];
        const LayerGrad& g = plan.lgrad[l];
        float* qkv = c.f(o.qkv); float* ctx = c.f(o.ctx); float* z1 = c.f(o.z1); float* hff = c.f(o.hff); float* z2 = c.f(o.z2);
        float* dyout = c.f(g.dyout); float* dz2 = c.f(g.dz2); float* dff = c.f(g.dz2d); float* dhff = c.f(g.dhff);
        float* dy1 = c.f(g.dy1); float* dz1 = c.f(g.dz1); float* dsa = c.f(g.dz1d); float* dqkv = c.f(g.dqkv); float* dctx = c.f(plan.dctx);
        // norm2: dz2 (residual gradient, flows to y1) and its dropped copy dff (gradient of the FFN output)
        {
            Section sl(ce.st, SEC_LN_BWD);
            TRY(bbbp_layernorm_bwd(ce.st, dyout, z2, PL(l, L_N2W), c.f(o.mean2), c.f(o.rstd2), dz2, plan.drop ? dff : nullptr,
                                   nullptr, nullptr, B, F, p_drop, site_seed(l, 3)));
        }
        // linear2 input gradient, then ReLU (+ dropout: hff is the post-dropout value, hff > 0 <=> active and kept)
        // the ReLU / dropout mask rides in the GEMM epilogue; the bias gradient (a column sum) is a leaf
        {
            Section sg(ce.st, SEC_FFN2_DGRAD);
            bbbp_gemm_desc gd = gemm_desc(0, 0, B, DFF, F, 1.f, dff, F, PL(l, L_W2), DFF, dhff, DFF);
            gd.gate = hff; gd.ldg = DFF; gd.gate_scale = inv_keep;
            TRY(bbbp_gemm_f32_grouped(ce.st, &gd, 1, ce.scratch(), ce.scratch_bytes()));
        }
        // leaves of this half layer (they only read per-layer buffers, so ONE event per half layer orders them all)
        TRY(leaf_after(ce));
        TRY(ffn_leaves(l, true));
        // dy1 = dhff W1 + dz2
        {
            Section sg(ce.st, SEC_FFN1_DGRAD);
            TRY(linear_bwd_input(ce, dhff, DFF, PL(l, L_W1), dy1, F, B, DFF, F, dz2, F));
        }
        // Layer 0 is the end of the pass: whatever its leaves still hold after the chain's last kernel is the step's tail.  Its LayerNorm
        // parameter gradients only need dyout and dy1, so they start here (one more event) instead of after the attention block.
        const bool ln_grads_early = l == 0 && ss != nullptr;
        if (ln_grads_early) { TRY(leaf_after(ce)); TRY(layer_norm_grads(l)); }
        // norm1
        {
            Section sl(ce.st, SEC_LN_BWD);
            TRY(bbbp_layernorm_bwd(ce.st, dy1, z1, PL(l, L_N1W), c.f(o.mean1), c.f(o.rstd1), dz1, plan.drop ? dsa : nullptr,
                                   nullptr, nullptr, B, F, p_drop, site_seed(l, 1)));
        }
        // out_proj input gradient (folded plan: dVW = Pd^T dsa and dPd = dsa VW^T take the out_proj output's gradient itself)
        if (!plan.fold) {
            Section sg(ce.st, SEC_OUTPROJ_DGRAD);
            TRY(linear_bwd_input(ce, dsa, F, PL(l, L_OUTW), dctx, F, B, F, F));
        }
        {
            Section sec_attn(ce.st, SEC_ATTN_BWD);
            if (plan.flash) {
                TRY(bbbp_attn_small_bwd(ce.st, qkv, ctx, c.f(o.lse), dctx, dqkv, B, F, NH, scale, p_drop, site_seed(l, 0), o.keep ? c.u8(o.keep) : nullptr));
            } else {
                TRY(attention_bwd_gemm(l, plan.fold ? dsa : dctx));
            }
        }
        TRY(leaf_after(ce));
        if (plan.fold) {
            TRY(folded_attn_leaves(l));
        } else {
            TRY(outproj_leaf(l, true));
            TRY(inproj_leaf(l, true));
        }
        if (ln_grads_early) TRY(record_layer_bucket(l));
        else TRY(layer_norm_leaves(l));
        if (l > 0 || d->need_input_grad) {
            Section sg(ce.st, SEC_QKV_DGRAD);
            TRY(linear_bwd_input(ce, dqkv, 3 * F, plan.fold ? c.f(plan.fwf[l]) : PL(l, L_INW), l > 0 ? c.f(plan.lgrad[l - 1].dyout) : c.f(plan.dA), F, B, 3 * F, F, dz1, F));
        }
        return BBBP_OK;
    }
};

// The forward step: fork; image branch; fingerprint branch; join; fusion block and head.
int forward_enqueue(void* stream, const bbbp_mixed_desc* d, const Plan& plan, const Schedule& s, const float* const* P, float* const* bn_running,
                    const float* fingerprint, const float* image, float* out, void* workspace) {
    SeedScope seed_scope(reinterpret_cast<const unsigned long long*>(static_cast<char*>(workspace) + plan.seed_slot));
    Step t(stream, d, plan, s, P, nullptr, fingerprint, image, workspace);
    // a deferred optimizer slice that is NOT this model's image-FC weight (another model's step, another tensor): wait before anything runs
    if (bbbp_param_pending_elsewhere(P[t.ix.ifc_w()])) (void)bbbp_param_wait(t.c.st, nullptr);
    TRY(t.fork(false));
    std::optional<Partition> part(std::in_place, t.ss != nullptr);           // ends early with reset(), or at any return
    TRY(t.image_fwd());          // enqueued first so the GPU is busy while the host feeds the encoder's launches
    {
        Section sec_enc(t.ce.st, SEC_ENCODER_FWD);
        if (s.enc_fwd == ENC_SLICED) TRY(t.encoder_fwd_sliced());
        else if (s.enc_fwd == ENC_ROWS) TRY(t.encoder_fwd_rows());
        else TRY(t.encoder_fwd_ops());
    }
    if (t.ss) TRY(join_side(t.c.st, t.ss));        // fusion needs both halves of `combined`
    part.reset();
    Section sec_head(t.c.st, SEC_HEAD_FWD);
    BBBP_CHECK_ARG(!plan.exact || s.head_fwd_fused, "the exact-global-batch mode needs the fused head (BBBP_FUSED_HEAD=1)");
    return s.head_fwd_fused ? t.head_fwd_fused(bn_running, out) : t.head_fwd_ops(bn_running, out);
}

// The backward step: fork; head and fusion block; image branch; fingerprint branch; join.  `plan`, `s`: as for forward_enqueue
int backward_enqueue(void* stream, const bbbp_mixed_desc* d, const Plan& plan, const Schedule& s, const float* const* P, float* const* G,
                     const float* fingerprint, const float* image, const float* dout, void* workspace) {
    SeedScope seed_scope(reinterpret_cast<const unsigned long long*>(static_cast<char*>(workspace) + plan.seed_slot));
    BBBP_CHECK_ARG(!plan.inference, "mixed_backward: the forward call used an inference workspace (desc.inference = 1)");
    (void)bbbp_param_wait(static_cast<hipStream_t>(stream), nullptr);      // (a deferred optimizer slice: normally consumed by the forward pass already)
    Step t(stream, d, plan, s, P, G, fingerprint, image, workspace);
    TRY(device_state(&t.ds));
    TRY(t.fork(true));
    std::optional<Section> sec;          // the caller's stream: head, then one section per kernel of the image branch
    sec.emplace(t.c.st, SEC_HEAD_BWD);
    BBBP_CHECK_ARG(!plan.exact || s.head_bwd_fused, "the exact-global-batch mode needs the fused head backward (bbbp_set_fused_head_bwd(1))");
    TRY(s.head_bwd_fused ? t.head_bwd_fused(dout) : t.head_bwd_ops(dout));
    // both branches only READ dcomb from here on
    if (t.ss) { TRY(after(t.ss, t.c.st, t.ce.st)); TRY(after(t.ss, t.c.st, t.cl.st)); }
    Partition part(t.ss != nullptr);
    TRY(t.image_bwd(sec));          // enqueued first: the host reaches its long kernels sooner
    if (s.head_bwd_fused) TRY(t.head_leaves(dout));
    Section sec_encb(t.ce.st, SEC_ENCODER_BWD);
    TRY(t.fingerprint_fc_leaf());
    if (s.enc_bwd == ENC_SLICED) TRY(t.encoder_bwd_sliced());
    else if (s.enc_bwd == ENC_ROWS) TRY(t.encoder_bwd_rows());
    else TRY(t.encoder_bwd_ops());
    if (t.ds) {
        // bucket 1 is final when the chain AND the leaves are: make the leaf stream wait for the chain's tail, record there
        if (t.ss) TRY(after(t.ss, t.ce.st, t.cl.st));
        TRY(record_bucket(t.ds->bucket1, t.cl.st));
    }
    if (t.ss) {
        TRY(join_side(t.c.st, t.ss));
        BBBP_CHECK_HIP(hipEventRecord(t.ss->join2, t.ss->leaf));
        BBBP_CHECK_HIP(hipStreamWaitEvent(t.c.st, t.ss->join2, 0));
    }
    return BBBP_OK;
}

hipStream_t capture_stream() {
    static hipStream_t cs = nullptr;       // captures never run on the caller's stream: the legacy default stream cannot be captured
    if (!cs && hipStreamCreateWithFlags(&cs, hipStreamNonBlocking) != hipSuccess) cs = nullptr;
    return cs;
}

// Run `enqueue(stream)` eagerly, or capture it on the library's capture stream and replay the graph on `st`.
template <typename F>
int run_or_replay(const GraphKey& key, hipStream_t st, F&& enqueue) {
    GraphEntry* slot = nullptr;
    const int mode = graph_lookup(key, &slot);
    if (mode == 2) {
        BBBP_CHECK_HIP(hipGraphLaunch(slot->exec, st));
        ++g_graph_replays;
        return BBBP_OK;
    }
    hipStream_t cs = mode == 1 ? capture_stream() : nullptr;
    if (cs && hipStreamBeginCapture(cs, hipStreamCaptureModeRelaxed) == hipSuccess) {
        const int rc = enqueue(cs);
        hipGraph_t graph = nullptr;
        const hipError_t e = hipStreamEndCapture(cs, &graph);
        bool ok = rc == BBBP_OK && e == hipSuccess && graph != nullptr;
        if (ok) ok = hipGraphInstantiate(&slot->exec, graph, nullptr, nullptr, 0) == hipSuccess;
        if (graph) (void)hipGraphDestroy(graph);
        if (ok) {
            slot->seen_only = false;
            ++g_graph_captures;
            BBBP_CHECK_HIP(hipGraphLaunch(slot->exec, st));
            return BBBP_OK;
        }
        (void)hipGetLastError();
        slot->exec = nullptr; slot->stamp = 0;       // do not try this key again soon; run it eagerly below
        if (rc) return rc;
    }
    return enqueue(st);
}

GraphKey make_key(int kind, const bbbp_mixed_desc* d, const Plan& plan, const Schedule& s, const void* a, const void* b, const void* c,
                  const void* ws, uint64_t phash) {
    GraphKey k{};
    k.kind = kind; k.d = *d; k.d.seed = 0;
    k.ptr[0] = a; k.ptr[1] = b; k.ptr[2] = c; k.ptr[3] = ws;
    k.phash = phash; k.s = s; k.fold = plan.fold; k.flash = plan.flash; k.attn_b3 = plan.attn_b3; k.total = plan.total; k.st = nullptr;
    return k;
}

}  // namespace

// Make `stream` wait until gradient bucket `bucket` of the most recent bbbp_mixed_backward on this device is final.
// bucket 0 = the image-FC weight (parameter index bbbp_mixed_bucket_param(d, 0)); bucket 1 = every parameter except
// that weight and the four conv tensors.  Returns BBBP_ERR_ARG when no such
// event exists (no backward yet, or the backward was replayed from a graph): the caller then waits for the whole stream.
extern "C" int bbbp_mixed_backward_wait_bucket(void* stream, int bucket) {
    BBBP_CHECK_ARG(bucket >= 0 && bucket < 2 + 32, "wait_bucket: unknown bucket %d", bucket);
    DeviceState* ds = nullptr; int dev = 0;
    TRY(device_state(&ds, &dev));
    BBBP_CHECK_ARG(ds, "wait_bucket: device %d", dev);
    const BucketEvent& b = bucket == 0 ? ds->bucket0 : bucket == 1 ? ds->bucket1 : ds->layer[bucket - 2];
    BBBP_CHECK_ARG(b.ev && b.recorded, "wait_bucket: no event for bucket %d on device %d", bucket, dev);
    BBBP_CHECK_HIP(hipStreamWaitEvent(static_cast<hipStream_t>(stream), b.ev, 0));
    return BBBP_OK;
}

// Make `stream` wait until the PARAMETERS of gradient bucket `bucket` may be overwritten: its gradient slice is final and this backward
// pass no longer reads those parameters (an optimizer step pipelined into the pass).  Bucket 0: after the image FC's input-gradient
// GEMM.  Layer l >= 1 (bucket 2 + l): when layer l - 1's bucket is final -- its leaves read what layer l's last kernel (the in_proj
// input gradient, the last reader of layer l's weights) wrote, and the leaf stream is in order, so layer l's own leaves are done too.
// Layer 0 and bucket 1 (everything but the conv tensors): the end of the fingerprint branch and its leaves (bucket 1's event).
extern "C" int bbbp_set_release_events(int on) {
    const int prev = g_release_events ? 1 : 0;
    g_release_events = on != 0;
    return prev;
}

extern "C" int bbbp_mixed_backward_wait_released(void* stream, int bucket) {
    BBBP_CHECK_ARG(bucket >= 0 && bucket < 2 + 32, "wait_released: unknown bucket %d", bucket);
    if (bucket == 0) {
        DeviceState* ds = nullptr; int dev = 0;
        TRY(device_state(&ds, &dev));
        BBBP_CHECK_ARG(ds && ds->bucket0.recorded && ds->bucket0_released.ev && ds->bucket0_released.recorded,
                       "wait_released: no event for bucket 0 on device %d (bbbp_set_release_events(1) before the backward pass)", dev);
        BBBP_CHECK_HIP(hipStreamWaitEvent(static_cast<hipStream_t>(stream), ds->bucket0_released.ev, 0));
        return BBBP_OK;
    }
    return bbbp_mixed_backward_wait_bucket(stream, bucket >= 3 ? bucket - 1 : 1);
}
__global__ void positive_gate_kernel(const float* x, uint8_t* gate, long n) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) gate[i] = x[i] > 0.f ? 1 : 0;
}
extern "C" int bbbp_mixed_debug_ffn_gate(void* stream, const bbbp_mixed_desc* d, const void* workspace, int layer, uint8_t* gate) {
    Plan plan;
    TRY(make_plan(d, &plan));
    BBBP_CHECK_ARG(workspace && gate, "debug_ffn_gate: null pointer");
    BBBP_CHECK_ARG(layer >= 0 && layer < plan.L, "debug_ffn_gate: layer %d of %d", layer, plan.L);
    BBBP_CHECK_ARG(!plan.inference, "debug_ffn_gate: an inference workspace keeps no per-layer activations");
    const long n = (long)plan.B * plan.DFF;
    const float* hff = reinterpret_cast<const float*>(static_cast<const char*>(workspace) + plan.layer[layer].hff);
    hipLaunchKernelGGL(positive_gate_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), hff, gate, n);
    BBBP_CHECK_LAUNCH();
    return BBBP_OK;
}
extern "C" int bbbp_mixed_debug_pool_mask(void* stream, const bbbp_mixed_desc* d, const void* workspace, int stage, uint8_t* mask) {
    Plan plan;
    TRY(make_plan(d, &plan));
    BBBP_CHECK_ARG(workspace && mask, "debug_pool_mask: null pointer");
    BBBP_CHECK_ARG(stage == 1 || stage == 2, "debug_pool_mask: stage %d (1 = conv1, 2 = conv2)", stage);
    BBBP_CHECK_ARG(!plan.inference, "debug_pool_mask: an inference workspace keeps no masks");
    const size_t n = stage == 1 ? (size_t)plan.B * C1 * (IMG / 2) * (IMG / 2) : (size_t)plan.B * IMG_FLAT;
    const char* src = static_cast<const char*>(workspace) + (stage == 1 ? plan.mask1 : plan.mask2);
    BBBP_CHECK_HIP(hipMemcpyAsync(mask, src, n, hipMemcpyDeviceToDevice, static_cast<hipStream_t>(stream)));
    return BBBP_OK;
}
extern "C" int bbbp_mixed_bucket_param(const bbbp_mixed_desc* d, int bucket) {
    if (!d || bucket != 0) return -1;
    return PIdx(d).ifc_w();
}
// first parameter index and tensor count of a bucket whose tensors are consecutive in params[] order (0: the image-FC weight;
// 2 + l: the twelve tensors of encoder layer l).  Bucket 1 (everything else) is not one range: returns -1.
extern "C" int bbbp_mixed_bucket_range(const bbbp_mixed_desc* d, int bucket, int* first, int* count) {
    if (!d || !first || !count || d->num_layers < 0 || d->num_layers > 32) return -1;
    const PIdx ix(d);
    if (bucket == 0) { *first = ix.ifc_w(); *count = 1; return 0; }
    if (bucket >= 2 && bucket < 2 + d->num_layers) { *first = ix.layer(bucket - 2, L_INW); *count = L_COUNT; return 0; }
    return -1;
}

extern "C" int bbbp_set_graphs(int on) { const int old = graphs_mode(); g_graphs_mode = on ? 1 : 0; return old; }

extern "C" int bbbp_graph_stats(long* captures, long* replays) {
    if (captures) *captures = g_graph_captures;
    if (replays) *replays = g_graph_replays;
    return BBBP_OK;
}

// The engine's side streams, events, profiling slots and graph cache are per-process state: enqueueing a forward or backward call is
// serialised (two host threads driving two models take turns ENQUEUEING, ~1 ms each; the GPU work itself overlaps as the streams allow).
static std::mutex g_engine_mutex;

extern "C" int bbbp_mixed_forward(void* stream, const bbbp_mixed_desc* d, const float* const* P, float* const* bn_running,
                                  const float* fingerprint, const float* image, float* out, void* workspace,
                                  size_t workspace_bytes) {
    std::lock_guard<std::mutex> engine_lock(g_engine_mutex);
    Plan plan;
    TRY(make_plan(d, &plan));
    const Schedule sched = make_schedule(plan, false);
    BBBP_CHECK_ARG(P && fingerprint && image && out && workspace && bn_running, "mixed_forward: null pointer");
    if (workspace_bytes < plan.total) { bbbp_set_error("mixed_forward: workspace %zu < %zu bytes", workspace_bytes, plan.total); return BBBP_ERR_WORKSPACE; }
    hipStream_t st = static_cast<hipStream_t>(stream);
    // the call's dropout seed goes to device memory first (never part of a graph: it changes every call)
    if (plan.drop) {
        hipLaunchKernelGGL(set_seed_kernel, dim3(1), dim3(1), 0, st,
                           reinterpret_cast<unsigned long long*>(static_cast<char*>(workspace) + plan.seed_slot), (unsigned long long)d->seed);
        BBBP_CHECK_LAUNCH();
    }
    const int np = PIdx(d).count();
    uint64_t h = hash_ptrs(reinterpret_cast<const void* const*>(P), np);
    h = hash_ptrs(reinterpret_cast<const void* const*>(bn_running), 2, h);
    const GraphKey key = make_key(0, d, plan, sched, fingerprint, image, out, workspace, h);
    auto enqueue = [&](hipStream_t s) { return forward_enqueue(s, d, plan, sched, P, bn_running, fingerprint, image, out, workspace); };
    return d->collective ? enqueue(st) : run_or_replay(key, st, enqueue);      // (host callbacks between the launches: nothing to capture)
}

extern "C" int bbbp_mixed_backward(void* stream, const bbbp_mixed_desc* d, const float* const* P, float* const* G,
                                   const float* fingerprint, const float* image, const float* dout, void* workspace,
                                   size_t workspace_bytes) {
    std::lock_guard<std::mutex> engine_lock(g_engine_mutex);
    Plan plan;
    TRY(make_plan(d, &plan));
    const Schedule sched = make_schedule(plan, true);
    BBBP_CHECK_ARG(P && G && fingerprint && image && dout && workspace, "mixed_backward: null pointer");
    if (workspace_bytes < plan.total) { bbbp_set_error("mixed_backward: workspace %zu < %zu bytes", workspace_bytes, plan.total); return BBBP_ERR_WORKSPACE; }
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int np = PIdx(d).count();
    uint64_t h = hash_ptrs(reinterpret_cast<const void* const*>(P), np);
    h = hash_ptrs(reinterpret_cast<const void* const*>(G), np, h);
    const GraphKey key = make_key(1, d, plan, sched, fingerprint, image, dout, workspace, h);
    auto enqueue = [&](hipStream_t s) { return backward_enqueue(s, d, plan, sched, P, G, fingerprint, image, dout, workspace); };
    return d->collective ? enqueue(st) : run_or_replay(key, st, enqueue);
}
