// A1: the BERT-base encoder forward that AspireConSent runs before pooling
// (examples/ex_aspire_consent.py:72-73: self.bert_encoder(tokid_tt, token_type_ids=seg_tt,
// attention_mask=attnmask_tt).last_hidden_state; the arithmetic itself is HuggingFace transformers'
// BertModel, pinned 4.5.1 in the reference's requirements.txt:14).
//
// Precision: the north star asks for sentence reps within 1e-4 of the fp32 CPU path through 12 layers: every GEMM is
// fp32-accurate.  The nn.Linear GEMMs (95 % of the flops) run on the 16-bit matrix pipes, every fp32 operand split into planes whose exact
// products are summed in fp32.  The default from 1024 token rows on, with the weights' planes prepared (aspire_bert_prepare_planes): two fp16
// planes formed once, three products per term (gemm_p_*_kernel; the layout and its error: enc_planes.h), and attention on the planes the QKV GEMM
// writes (flash_attn_p_kernel).  Below that, or without planes: three bf16 planes split on the fly and six products per term
// (gemm_bf16x3_kernel: same error against float64 as the fp32-input MFMA, 1.4-1.6x its speed), and flash_attn_f16x2_kernel, which splits fp32
// Q / K / V itself.  The A/B forms (ASPIRE_HIP_GEMM=f32: gemm_f32_kernel, ASPIRE_HIP_ATTN=f32: flash_attn_f32_kernel) use the fp32-input matrix
// cores (v_mfma_f32_32x32x2_f32: exact fp32 FMA chains, 157 TFLOP/s peak on MI355X -- still the figure the encoder's
// throughput is quoted against, so the split forms can exceed 100 % of it).  Plain bf16 inputs give ~1e-2: not an option.
//
// A1d: the same forward for the BERT-shaped encoders of the SentenceTransformer baselines (src/evaluation/utils/models.py:379-410:
// SentenceModel.encode = SentenceTransformer(name).encode; RobertaModel, MPNetModel): aspire_bert_forward_var_f32 takes the position
// row of every token from a table (aspire_bert_extras::pos_ids) and adds MPNet's relative-position bias to the attention scores
// (::rel_bias); without either it is aspire_bert_forward_f32 launch for launch.  The masked-mean read-out behind it is pool.hip's.
//
// This file is host only: the workspace, the forward's plan (plan_forward), one layer of it (run_layer: the plane path here, otherwise the
// fp32-operand body of enc_host.h), the CLS forward and the C entry
// points (aspire_bert_status and the clock build's aspire_debug_gemm_buffer sit with their device globals in enc_gemm_p.hip).  The kernels and their launch rules, one unit per family, each
// kernel launched from one host function of its unit (enc_types.h declares them):
//   enc_gemm.hip     gemm_f32_kernel, gemm_bf16x3_kernel: GEMMs on fp32 operands                              launch_gemm
//   enc_gemm_p.hip   split_planes_kernel, gemm_p_kernel, gemm_p_w8_kernel, gemm_p_qkv_kernel, gemm_p_ln_kernel:
//                    GEMMs on pre-split fp16 planes                                                          launch_gemm_p, _qkv, _ln, launch_split_planes
//   enc_gemm_h.hip   split_h_kernel, layernorm_h_kernel, gemm_h_kernel: the opt-in fp16 matmul mode's GEMM on
//                    single-plane fp16 operands (ASPIRE_MATMUL_FP16, the _prec entries)                      launch_gemm_h, launch_split_h, launch_layernorm_h
//   enc_attn.hip     flash_attn_p_kernel, flash_attn_p64_kernel, flash_attn_f16x2_kernel, flash_attn_f32_kernel,
//                    softmax_mask_kernel, cls_attn_kernel                                                    launch_flash_attn_p, launch_flash_attn, launch_softmax_mask, launch_cls_attn
//   enc_rows.hip     layernorm_kernel, embed_layernorm_kernel, cls_tap_kernel                                launch_layernorm, launch_embed_layernorm, launch_cls_tap
//   enc_pooler.hip   bert_pooler_kernel: tanh(cls . W^T + b) behind the CLS forward (aspire_bert_pooler_f32)   launch_pooler
//   enc_planes.h     the fp16-plane layout: constants and device helpers; enc_hplane.h: the single-plane layout of the fp16 matmul mode
//   enc_host.h       host only, shared with encoder_bwd.hip: the buffer carver, the GemmArgs builders (linear, head_gemm), the three-kernel
//                    attention (attention_gemm), the fp32-operand layer tail (layer_tail), the geometry and null-pointer checks
// The layer stack under training (the tape-keeping forward over the same enc_host.h launches, and the backward) has a host file of
// its own, encoder_bwd.hip, with its row kernels in enc_bwd.hip and the TN GEMM form in enc_gemm.hip (launch_gemm_tn).
#include <math.h>

#include "enc_host.h"
#include "enc_hplane.h"
#include "enc_planes.h"
#include "tuning.h"

namespace aspire {
namespace {

struct Workspace {
    float *x, *qkv, *scores, *ctx, *tmp, *ffn;
    void *actp, *ctxp, *ffnp;       // P-layout activations (pre-split GEMM operands): LayerNorm outputs, attention context, GELU(FFN1);
                                    // the fp16 matmul mode keeps its H-layout activations (half the bytes: enc_hplane.h) in the same slots
    float2* ln_stats;               // the LayerNorm-epilogue GEMMs' per-row, per-column-tile moments [M][12]
    int* ln_count;                  // their arrival counters [2 n_layers][row blocks], zeroed once per forward
    size_t ln_count_bytes;
    unsigned char* qkvp;            // round 6: the attention's operands as the QKV GEMM splits them (flash_attn_p_kernel): [plane][Q | K | V][head][M][64] fp16
    size_t total;
};

Workspace carve(void* base, int64_t B, int64_t L, int heads, int ffn_dim, int n_layers) {
    const size_t M = (size_t)B * L, Lp = (size_t)(L + 3) / 4 * 4;
    Carver c(base);
    Workspace w;
    w.x = c.floats(M * kD);
    w.qkv = c.floats(M * 3 * kD);
    w.scores = c.floats((size_t)B * heads * L * Lp);
    w.ctx = c.floats(M * kD);
    w.tmp = c.floats(M * kD);
    w.ffn = c.floats(M * ffn_dim);
    w.actp = c.bytes(p_bytes((int64_t)M, kD));
    w.ctxp = c.bytes(p_bytes((int64_t)M, kD));
    w.ffnp = c.bytes(p_bytes((int64_t)M, ffn_dim));
    w.ln_stats = reinterpret_cast<float2*>(c.floats(M * 24));
    w.ln_count_bytes = (size_t)2 * (n_layers > 0 ? n_layers : 0) * ((M + 127) / 128) * sizeof(int);
    w.ln_count = reinterpret_cast<int*>(c.floats(w.ln_count_bytes / sizeof(float) + 1));
    w.qkvp = reinterpret_cast<unsigned char*>(c.floats(M * 3 * kD));                 // 2 planes x [Q | K | V] x M x 768 fp16 = the bytes of the fp32 qkv
    w.total = c.off;
    return w;
}

// where a layer's four weight matrices sit in the prepared planes buffer
struct PlaneOffsets {
    size_t qkv, o, ffn1, ffn2, per_layer;
};
PlaneOffsets plane_offsets(int ffn_dim) {
    PlaneOffsets o{};
    Carver c(nullptr);
    o.qkv = c.off; c.bytes(p_bytes(3 * kD, kD));
    o.o = c.off; c.bytes(p_bytes(kD, kD));
    o.ffn1 = c.off; c.bytes(p_bytes(ffn_dim, kD));
    o.ffn2 = c.off; c.bytes(p_bytes(kD, ffn_dim));
    o.per_layer = c.off;
    return o;
}

// ... and in the H planes of the fp16 matmul mode (aspire_bert_prepare_hplanes)
PlaneOffsets hplane_offsets(int ffn_dim) {
    PlaneOffsets o{};
    Carver c(nullptr);
    o.qkv = c.off; c.bytes(h_bytes(3 * kD, kD));
    o.o = c.off; c.bytes(h_bytes(kD, kD));
    o.ffn1 = c.off; c.bytes(h_bytes(ffn_dim, kD));
    o.ffn2 = c.off; c.bytes(h_bytes(kD, ffn_dim));
    o.per_layer = c.off;
    return o;
}

// ---------------------------------------------------------------------------------------------------------------
// One forward's plan -- the form every step takes, decided once from B, L, the weights and the tuning pins -- and one layer of it.
// aspire_bert_forward_f32 runs every layer through run_layer; aspire_bert_forward_cls_f32 runs all but the last one the same way.
// ---------------------------------------------------------------------------------------------------------------
struct Fwd {
    const aspire_bert_weights* w;
    const int64_t* mask;
    const int64_t* pos_ids;         // aspire_bert_extras (forward_var): NULL = BertModel's positions / no bias
    const float* rel_bias;
    int rel_span;
    int64_t B, L, M, row_tiles;
    int Lp, H, dh;
    bool pp, ln_fused, attn_p;
    bool hh;                        // the fp16 matmul mode: the four projections on H operands (run_layer's H path), at every M
    const void* hplanes;
    PlaneOffsets po, ho;
    Workspace ws;
    hipStream_t st;
};

// the forwards' argument checks: all of them before the first launch
int check_forward_args(const aspire_bert_weights* w, const int64_t* tok_ids, const int64_t* attn_mask, const float* out, int64_t B, int64_t L) {
    ASPIRE_REQUIRE(w && tok_ids && attn_mask && out, ASPIRE_ERR_INVALID_ARG, "null pointer");
    if (int rc = check_bert_shape(w, B, L)) return rc;
    ASPIRE_REQUIRE(L <= w->max_pos, ASPIRE_ERR_INVALID_ARG, "sequence length %lld beyond max_position_embeddings=%d", (long long)L, w->max_pos);
    return ASPIRE_OK;
}

int plan_forward(Fwd& f, const aspire_bert_weights* w, const int64_t* attn_mask, int64_t B, int64_t L, void* workspace, hipStream_t st,
                 const void* hplanes = nullptr, int matmul = ASPIRE_MATMUL_FP32) {
    f.w = w;
    f.mask = attn_mask;
    f.pos_ids = nullptr;
    f.rel_bias = nullptr;
    f.rel_span = 0;
    f.B = B;
    f.L = L;
    f.st = st;
    f.ws = carve(workspace, B, L, w->n_heads, w->ffn_dim, w->n_layers);
    f.M = B * L;
    f.Lp = (int)((L + 3) / 4 * 4);
    f.H = w->n_heads;
    f.dh = kD / f.H;
    // P path: the weights' planes are prepared (aspire_bert_prepare_planes), BERT-base shapes tile by 128 -- every nn.Linear GEMM
    // streams pre-split fp16 operands (gemm_p_kernel), from 1024 token rows on (measured B x L = 4 x 128: 2.46 vs 2.42 ms per batch,
    // 8 x 128: 2.55 vs 2.81, 16 x 128: 2.90 vs 3.52, 32 x 256: 6.64 vs 9.8); below -- and with ASPIRE_HIP_GEMM=f32 | bf16x3, or without
    // planes -- the round-2 kernels, which pick smaller tiles for small M
    f.pp = w->planes != nullptr && (tuning().gemm_form == 0 ? f.M >= 1024 : tuning().gemm_form == 3) && f.dh == 64 && !tuning().attn_gemm &&
           w->ffn_dim % 128 == 0;
    f.po = plane_offsets(w->ffn_dim);
    // LayerNorm in the N = 768 GEMMs' epilogue (ASPIRE_HIP_GEMM_LN=off: the separate layernorm_kernel pass)
    // from 48 row tiles on (measured, fused / separate ms per batch: 64 x 256 9.00 - 9.18 / 9.45, 128 x 128 8.99 / 9.40, 64 x 128 5.05 / 5.15,
    // 32 x 256 5.16 / 5.30, 40 x 100 3.09 / 3.17, 16 x 256 3.18 / 3.14, 8 x 256 2.37 / 2.30: below, the launch is a fraction of one round of
    // workgroups and a waiting workgroup has nothing running under it)
    f.row_tiles = (f.M + 127) / 128;
    f.ln_fused = f.pp && (tuning().gemm_ln == 2 || (tuning().gemm_ln == 0 && f.row_tiles >= 48 && ln_fused_supported()));
    // Round 6 (default on the plane path; ASPIRE_HIP_ATTN=f16x2 pins round 5's form, which splits fp32 Q / K / V inside the attention kernel):
    // the QKV GEMM writes the attention's operands as fp16 planes, the attention stages them by LDS-DMA (flash_attn_p_kernel)
    f.attn_p = f.pp && w->n_layers > 0 && tuning().attn_form != 1 && !tuning().attn_f32 && tuning().gemm_tile == 0;
    // The fp16 matmul mode (ASPIRE_MATMUL_FP16, opt-in): every nn.Linear operand rounded to fp16 once, one product per term
    // (gemm_h_kernel), at EVERY M -- the mode has no 1024-row threshold (below it neither path has been measured in this mode).  A
    // GEMM pin (ASPIRE_HIP_GEMM=..) overrides the mode: run_checked re-encodes an overflowed forward under GEMM=bf16x3, and the plan
    // above then holds as it stands.  The residual stream, LayerNorm and the attention stay fp32 launches: fp32 x exists at every layer
    f.hplanes = hplanes;
    f.ho = hplane_offsets(w->ffn_dim);
    f.hh = matmul == ASPIRE_MATMUL_FP16 && hplanes != nullptr && w->n_layers > 0 && f.dh == 64 && w->ffn_dim % 128 == 0 && tuning().gemm_form == 0;
    if (f.hh) f.pp = f.ln_fused = f.attn_p = false;
    return ASPIRE_OK;
}

// embeddings + LayerNorm -> x (fp32) and, on the P path, actp; then the LayerNorm-epilogue counters of this forward
int launch_embed(const Fwd& f, const int64_t* tok_ids, const int64_t* type_ids, float* x) {
    const aspire_bert_weights* w = f.w;
    if (int rc = launch_embed_layernorm(tok_ids, type_ids, f.pos_ids, w->word_emb, w->pos_emb, w->type_emb, w->emb_ln_g, w->emb_ln_b, w->ln_eps, x, f.M, f.L,
                                        f.pp && w->n_layers > 0 ? f.ws.actp : nullptr, f.st))
        return rc;
    // the P layout's slot offsets are 32-bit byte offsets (p_slot / p_slot8: ((k >> 4) R + r) << 6): the widest operand is [M, ffn_dim]
    ASPIRE_REQUIRE(!f.pp || (uint64_t)f.M * (uint64_t)(w->ffn_dim > 3 * kD ? w->ffn_dim : 3 * kD) * 4 < (1ull << 32), ASPIRE_ERR_UNSUPPORTED,
                   "%lld token rows in one forward: the fp16-plane layout addresses < 4 GB per operand (split the batch)", (long long)f.M);
    if (f.ln_fused && w->n_layers > 0) ASPIRE_HIP_OK(hipMemsetAsync(f.ws.ln_count, 0, f.ws.ln_count_bytes, f.st));
    if (f.hh) {
        // the H layout's slot offsets are 32-bit byte offsets too (h_slot8): 2 bytes per element
        ASPIRE_REQUIRE((uint64_t)f.M * (uint64_t)(w->ffn_dim > 3 * kD ? w->ffn_dim : 3 * kD) * 2 < (1ull << 32), ASPIRE_ERR_UNSUPPORTED,
                       "%lld token rows in one forward: the fp16-plane layout addresses < 4 GB per operand (split the batch)", (long long)f.M);
        // the embedding LayerNorm's fp32 rows go through split_h_kernel (no fused H writer in embed_layernorm_kernel)
        if (int rc = launch_split_h(x, f.M, kD, kD, f.ws.actp, false, nullptr, f.st)) return rc;
    }
    return ASPIRE_OK;
}

// layer l: x (its input, fp32; on the fused form the input lives in actp) -> out.  last: out is the caller's [M, 768] and no P copy of
// it is written.  qkv_only: step 1 alone (the CLS forward's last layer)
int run_layer(const Fwd& f, int l, const float* x, float* out, bool last, bool qkv_only) {
    const aspire_bert_weights* w = f.w;
    const Workspace& ws = f.ws;
    const PlaneOffsets& po = f.po;
    const bool pp = f.pp, ln_fused = f.ln_fused, attn_p = f.attn_p;
    const int64_t B = f.B, L = f.L, M = f.M, row_tiles = f.row_tiles;
    const int Lp = f.Lp, H = f.H, dh = f.dh;
    const int64_t* attn_mask = f.mask;
    hipStream_t st = f.st;
    const aspire_bert_layer& ly = w->layers[l];
    if (f.hh) {
        // The fp16 matmul mode: the !ln_fused plane route below with H buffers where it has P buffers (the workspace's P slots hold them)
        const PlaneOffsets& ho = f.ho;
        const char* lh = (const char*)f.hplanes + (size_t)l * ho.per_layer;
        // 1. QKV projection -> fp32 qkv
        HGemmArgs hg{ws.actp, lh + ho.qkv, ws.qkv, nullptr, ly.b_qkv, nullptr, (int)M, 3 * kD, kD, 3 * kD, 0, 0};
        if (int rc = launch_gemm_h(hg, false, st)) return rc;
        if (qkv_only) return ASPIRE_OK;
        // 2-4. attention: an existing kernel on fp32 Q / K / V, unchanged; its fp32 context goes to H through split_h_kernel
        if (!tuning().attn_gemm) {
            if (int rc = launch_flash_attn(ws.qkv, attn_mask, ws.ctx, B, (int)L, H, nullptr, M, tuning().attn_f32 != 0, f.rel_bias, f.rel_span, st)) return rc;
        } else {
            if (int rc = attention_gemm(ws.qkv, ws.scores, ws.ctx, attn_mask, B, L, Lp, H, dh, f.rel_bias, f.rel_span, st)) return rc;
        }
        if (int rc = launch_split_h(ws.ctx, M, kD, kD, ws.ctxp, false, nullptr, st)) return rc;
        // 5. attention output projection + fp32 residual, LayerNorm -> h (fp32 ws.ctx and its H copy)
        hg = HGemmArgs{ws.ctxp, lh + ho.o, ws.tmp, nullptr, ly.b_o, x, (int)M, kD, kD, kD, kD, 0};
        if (int rc = launch_gemm_h(hg, false, st)) return rc;
        if (int rc = launch_layernorm_h(ws.tmp, ly.ln1_g, ly.ln1_b, w->ln_eps, ws.ctx, M, ws.actp, st)) return rc;
        // 6. FFN: GELU(h . W1^T + b1) straight into the H layout (no fp32 [M, ffn] exists), . W2^T + b2 + h, LayerNorm
        hg = HGemmArgs{ws.actp, lh + ho.ffn1, nullptr, ws.ffnp, ly.b_ffn1, nullptr, (int)M, w->ffn_dim, kD, 0, 0, 0};
        if (int rc = launch_gemm_h(hg, true, st)) return rc;
        hg = HGemmArgs{ws.ffnp, lh + ho.ffn2, ws.tmp, nullptr, ly.b_ffn2, ws.ctx, (int)M, kD, w->ffn_dim, kD, kD, 0};
        if (int rc = launch_gemm_h(hg, false, st)) return rc;
        return launch_layernorm_h(ws.tmp, ly.ln2_g, ly.ln2_b, w->ln_eps, out, M, last ? nullptr : ws.actp, st);
    }
    const char* lp = (const char*)w->planes + (size_t)l * po.per_layer;
    PGemmArgs pg{};
    // 1. fused QKV projection: qkv [M, 2304] = x . Wqkv^T + bqkv
    if (attn_p) {
        // Q, K and V go out as the attention kernel's fp16 planes (no fp32 qkv exists in this form)
        pg = PGemmArgs{ws.actp, lp + po.qkv, nullptr, nullptr, ly.b_qkv, nullptr, (int)M, 3 * kD, kD, 0, 0, 0};
        pg.Xp = ws.qkvp;
        if (int rc = launch_gemm_p_qkv(pg, st)) return rc;
    } else if (pp) {
        pg = PGemmArgs{ws.actp, lp + po.qkv, ws.qkv, nullptr, ly.b_qkv, nullptr, (int)M, 3 * kD, kD, 3 * kD, 0, 0};
        if (int rc = launch_gemm_p(pg, false, st)) return rc;
    } else {
        if (int rc = launch_gemm(linear(x, ly.w_qkv, ws.qkv, ly.b_qkv, nullptr, M, 3 * kD, kD), 1, false, st)) return rc;
    }
    if (qkv_only) return ASPIRE_OK;
    // 2-4. attention.  Fused kernel (scores never leave the chip) unless ASPIRE_HIP_ATTN=gemm pins the
    // three-kernel form (QK^T GEMM, masked soft-max, PV GEMM) that the fused one is tested against.
    if (attn_p) {
        if (int rc = launch_flash_attn_p(ws.qkvp, attn_mask, ws.ctx, B, (int)L, H, ws.ctxp, M, tuning().attn_form == 2, f.rel_bias, f.rel_span, st))
            return rc;
    } else if (dh == 64 && !tuning().attn_gemm) {
        if (int rc = launch_flash_attn(ws.qkv, attn_mask, ws.ctx, B, (int)L, H, pp ? ws.ctxp : nullptr, M, tuning().attn_f32 != 0, f.rel_bias,
                                       f.rel_span, st))
            return rc;
    } else {
        if (int rc = attention_gemm(ws.qkv, ws.scores, ws.ctx, attn_mask, B, L, Lp, H, dh, f.rel_bias, f.rel_span, st)) return rc;
    }
    // 5-6 on fp32 operands: the shared body.  h = LN1(.) goes where the context was read from, both pre-norm sums to ws.tmp
    if (!pp) return layer_tail(w, ly, ws.ctx, x, TailSlots{ws.tmp, ws.ctx, nullptr, ws.ffn, ws.tmp}, out, M, st);
    // ... and on the planes:
    // 5. attention output projection + residual, LayerNorm
    if (ln_fused) {
        // x lives in actp (written by the embedding LayerNorm / the previous layer's FFN2 epilogue, read by the QKV GEMM): read as the
        // residual and replaced by h = LN1(.) slot by slot; no fp32 copy of x or h exists in this form
        pg = PGemmArgs{ws.ctxp, lp + po.o, nullptr, ws.actp, ly.b_o, nullptr, (int)M, kD, kD, kD, kD, 0};
        pg.resp = ws.actp;
        pg.gamma = ly.ln1_g; pg.beta = ly.ln1_b; pg.eps = w->ln_eps;
        pg.ln_stats = ws.ln_stats; pg.ln_count = ws.ln_count + (size_t)(2 * l) * row_tiles;
        if (int rc = launch_gemm_p_ln(pg, st)) return rc;
    } else {
        pg = PGemmArgs{ws.ctxp, lp + po.o, ws.tmp, nullptr, ly.b_o, x, (int)M, kD, kD, kD, kD, 0};
        if (int rc = launch_gemm_p(pg, false, st)) return rc;
        if (int rc = launch_layernorm(ws.tmp, ly.ln1_g, ly.ln1_b, w->ln_eps, ws.ctx, M, ws.actp, st)) return rc;
    }
    // 6. FFN: GELU(h . W1^T + b1) . W2^T + b2 + h, LayerNorm          (h = ws.ctx)
    pg = PGemmArgs{ws.actp, lp + po.ffn1, nullptr, ws.ffnp, ly.b_ffn1, nullptr, (int)M, w->ffn_dim, kD, 0, 0, 0};
    if (int rc = launch_gemm_p(pg, true, st)) return rc;
    if (ln_fused) {
        pg = PGemmArgs{ws.ffnp, lp + po.ffn2, last ? out : nullptr, last ? nullptr : ws.actp, ly.b_ffn2, nullptr, (int)M, kD, w->ffn_dim, kD, kD, 0};
        pg.resp = ws.actp;
        pg.gamma = ly.ln2_g; pg.beta = ly.ln2_b; pg.eps = w->ln_eps;
        pg.ln_stats = ws.ln_stats; pg.ln_count = ws.ln_count + (size_t)(2 * l + 1) * row_tiles;
        return launch_gemm_p_ln(pg, st);
    }
    pg = PGemmArgs{ws.ffnp, lp + po.ffn2, ws.tmp, nullptr, ly.b_ffn2, ws.ctx, (int)M, kD, w->ffn_dim, kD, kD, 0};
    if (int rc = launch_gemm_p(pg, false, st)) return rc;
    return launch_layernorm(ws.tmp, ly.ln2_g, ly.ln2_b, w->ln_eps, out, M, last ? nullptr : ws.actp, st);
}

// The CLS forward's own workspace, behind the forward's (carve): the B gathered rows of the last layer
struct ClsWorkspace {
    float *gin, *ctx, *tmp, *h, *y, *ffn;      // residual input (hidden state n - 1), attention context, pre-norm, LN1, LN2, GELU(FFN1)
    size_t total;
};
ClsWorkspace carve_cls(void* base, int64_t B, int ffn_dim) {
    Carver cv(base);
    ClsWorkspace c;
    c.gin = cv.floats((size_t)B * kD);
    c.ctx = cv.floats((size_t)B * kD);
    c.tmp = cv.floats((size_t)B * kD);
    c.h = cv.floats((size_t)B * kD);
    c.y = cv.floats((size_t)B * kD);
    c.ffn = cv.floats((size_t)B * ffn_dim);
    c.total = cv.off;
    return c;
}

}  // namespace
}  // namespace aspire

using namespace aspire;

extern "C" size_t aspire_bert_workspace_bytes(const aspire_bert_weights* w, int64_t B, int64_t L) {
    if (!w || B <= 0 || L <= 0) return 0;
    return carve(nullptr, B, L, w->n_heads, w->ffn_dim, w->n_layers).total;
}

// BertModel's forward is the forward below without extras: one body, so the two cannot drift apart
extern "C" int aspire_bert_forward_f32(const aspire_bert_weights* w, const int64_t* tok_ids, const int64_t* type_ids,
                                       const int64_t* attn_mask, int64_t B, int64_t L, float* hidden_out, void* workspace,
                                       size_t workspace_bytes, void* stream) {
    return aspire_bert_forward_var_f32(w, nullptr, tok_ids, type_ids, attn_mask, B, L, hidden_out, workspace, workspace_bytes, stream);
}

// the _prec entries' mode check: ASPIRE_MATMUL_FP32, or ASPIRE_MATMUL_FP16 with the weights' H planes; no device is touched
static int check_matmul_mode(int matmul, const void* hplanes) {
    ASPIRE_REQUIRE(matmul == ASPIRE_MATMUL_FP32 || matmul == ASPIRE_MATMUL_FP16, ASPIRE_ERR_INVALID_ARG,
                   "matmul mode %d: the inference forwards take ASPIRE_MATMUL_FP32 (0) or ASPIRE_MATMUL_FP16 (4)", matmul);
    ASPIRE_REQUIRE(matmul != ASPIRE_MATMUL_FP16 || hplanes, ASPIRE_ERR_INVALID_ARG,
                   "ASPIRE_MATMUL_FP16 without hplanes (aspire_bert_prepare_hplanes)");
    return ASPIRE_OK;
}

extern "C" int aspire_bert_forward_var_f32(const aspire_bert_weights* w, const aspire_bert_extras* x_, const int64_t* tok_ids,
                                           const int64_t* type_ids, const int64_t* attn_mask, int64_t B, int64_t L, float* hidden_out,
                                           void* workspace, size_t workspace_bytes, void* stream) {
    return aspire_bert_forward_prec_f32(w, x_, nullptr, ASPIRE_MATMUL_FP32, tok_ids, type_ids, attn_mask, B, L, hidden_out, workspace,
                                        workspace_bytes, stream);
}

// The forward in a matmul mode: with ASPIRE_MATMUL_FP32 the body every forward above always ran (hplanes is not read)
extern "C" int aspire_bert_forward_prec_f32(const aspire_bert_weights* w, const aspire_bert_extras* x_, const void* hplanes, int matmul,
                                            const int64_t* tok_ids, const int64_t* type_ids, const int64_t* attn_mask, int64_t B, int64_t L,
                                            float* hidden_out, void* workspace, size_t workspace_bytes, void* stream) {
    if (int rc = check_forward_args(w, tok_ids, attn_mask, hidden_out, B, L)) return rc;
    if (int rc = check_matmul_mode(matmul, hplanes)) return rc;
    ASPIRE_REQUIRE(!x_ || !x_->rel_bias || x_->rel_span >= L, ASPIRE_ERR_INVALID_ARG,
                   "rel_span %d < sequence length %lld: the bias table does not cover every (query, key) distance", x_ ? x_->rel_span : 0,
                   (long long)L);
    if (B == 0) return ASPIRE_OK;
    const size_t need = carve(nullptr, B, L, w->n_heads, w->ffn_dim, w->n_layers).total;
    ASPIRE_REQUIRE(workspace && workspace_bytes >= need, ASPIRE_ERR_INVALID_ARG, "workspace too small: need %zu bytes", need);
    Fwd f;
    if (int rc = plan_forward(f, w, attn_mask, B, L, workspace, (hipStream_t)stream, hplanes, matmul)) return rc;
    if (x_) {
        f.pos_ids = x_->pos_ids;
        f.rel_bias = x_->rel_bias;
        f.rel_span = x_->rel_bias ? x_->rel_span : 0;
    }
    // (the 64-key attention form is not built with the bias: refused here, before the embedding launch, not in layer 0)
    ASPIRE_REQUIRE(!(f.rel_bias && f.attn_p && tuning().attn_form == 2), ASPIRE_ERR_UNSUPPORTED,
                   "the 64-key attention form (ASPIRE_HIP_ATTN=p64) is not built with a relative-position bias");
    float* x = w->n_layers == 0 ? hidden_out : f.ws.x;
    if (int rc = launch_embed(f, tok_ids, type_ids, x)) return rc;
    for (int l = 0; l < w->n_layers; ++l) {
        const bool last = l == w->n_layers - 1;
        float* out = last ? hidden_out : f.ws.x;  // LN2 writes the layer output (x is dead by then)
        if (int rc = run_layer(f, l, x, out, last, false)) return rc;
        x = out;
    }
    return ASPIRE_OK;
}

extern "C" size_t aspire_bert_cls_workspace_bytes(const aspire_bert_weights* w, int64_t B, int64_t L) {
    if (!w || B <= 0 || L <= 0) return 0;
    const size_t base = carve(nullptr, B, L, w->n_heads, w->ffn_dim, w->n_layers).total;
    return base + carve_cls(nullptr, B, w->ffn_dim).total;
}

// The CLS rows of every hidden state and their mix (ex_aspire_bienc.py:23-58, disent_models.py:183-205): layers 0 .. n - 2 are
// aspire_bert_forward_f32's own launches; after the embedding LayerNorm and after every layer cls_tap_kernel reads the B CLS rows
// where that form left them (fp32 x, or the fp16 planes of actp on the fused-LayerNorm form) and adds w_l x row to cls_out.  The last
// layer runs its QKV GEMM over all rows, then ONE query per (document, head) (cls_attn_kernel) and the rest of the layer on the B
// gathered rows only: nothing after the keys and values of a non-CLS row is ever read.
extern "C" int aspire_bert_forward_cls_f32(const aspire_bert_weights* w, const int64_t* tok_ids, const int64_t* type_ids,
                                           const int64_t* attn_mask, int64_t B, int64_t L, const float* layer_mix, float* cls_out,
                                           float* layer_cls, void* workspace, size_t workspace_bytes, void* stream) {
    return aspire_bert_forward_cls_prec_f32(w, nullptr, ASPIRE_MATMUL_FP32, tok_ids, type_ids, attn_mask, B, L, layer_mix, cls_out, layer_cls,
                                            workspace, workspace_bytes, stream);
}

// ... in a matmul mode.  ASPIRE_MATMUL_FP16: layers 0 .. n - 2 and the last layer's QKV GEMM run in the mode; the last layer's tail on
// the B CLS rows (one query per document and head, then layer_tail) is the existing fp32 one
extern "C" int aspire_bert_forward_cls_prec_f32(const aspire_bert_weights* w, const void* hplanes, int matmul, const int64_t* tok_ids,
                                                const int64_t* type_ids, const int64_t* attn_mask, int64_t B, int64_t L,
                                                const float* layer_mix, float* cls_out, float* layer_cls, void* workspace,
                                                size_t workspace_bytes, void* stream) {
    if (int rc = check_forward_args(w, tok_ids, attn_mask, cls_out, B, L)) return rc;
    if (int rc = check_matmul_mode(matmul, hplanes)) return rc;
    if (layer_mix)
        for (int i = 0; i <= w->n_layers; ++i)
            ASPIRE_REQUIRE(isfinite(layer_mix[i]), ASPIRE_ERR_INVALID_ARG, "layer_mix[%d] is not finite", i);
    if (B == 0) return ASPIRE_OK;
    const size_t need = aspire_bert_cls_workspace_bytes(w, B, L);
    ASPIRE_REQUIRE(workspace && workspace_bytes >= need, ASPIRE_ERR_INVALID_ARG, "workspace too small: need %zu bytes", need);
    Fwd f;
    if (int rc = plan_forward(f, w, attn_mask, B, L, workspace, (hipStream_t)stream, hplanes, matmul)) return rc;
    const ClsWorkspace cw = carve_cls((char*)workspace + f.ws.total, B, w->ffn_dim);
    const int n = w->n_layers;
    // hidden state i: its CLS row -> layer_cls[i], cls_out (+)= mix[i] x row, and (i = n - 1) the last layer's residual input
    auto tap = [&](int i, const float* x, const void* xp, int64_t rows, int64_t ld_rows) -> int {
        const int mode = layer_mix ? (i == 0 ? 1 : 2) : (i == n ? 1 : 0);
        const float wt = layer_mix ? layer_mix[i] : 1.f;
        return launch_cls_tap(x, xp, rows, ld_rows, B, wt, mode, cls_out, layer_cls ? layer_cls + (size_t)i * B * kD : nullptr,
                              i == n - 1 ? cw.gin : nullptr, f.st);
    };
    if (int rc = launch_embed(f, tok_ids, type_ids, f.ws.x)) return rc;
    if (int rc = tap(0, f.ws.x, nullptr, f.M, L)) return rc;
    for (int l = 0; l + 1 < n; ++l) {
        if (int rc = run_layer(f, l, f.ws.x, f.ws.x, false, false)) return rc;
        // the fused form keeps a layer's output only as the planes of actp; the others write fp32 x
        if (int rc = f.ln_fused ? tap(l + 1, nullptr, f.ws.actp, f.M, L) : tap(l + 1, f.ws.x, nullptr, f.M, L)) return rc;
    }
    if (n == 0) return ASPIRE_OK;
    // the last layer: Q, K, V of every row as the forward's attention form lays them out ...
    const aspire_bert_layer& ly = w->layers[n - 1];
    if (int rc = run_layer(f, n - 1, f.ws.x, f.ws.x, true, true)) return rc;
    if (int rc = launch_cls_attn(f.attn_p ? nullptr : f.ws.qkv, f.attn_p ? f.ws.qkvp : nullptr, attn_mask, cw.ctx, B, (int)L, f.H, f.M, f.st))
        return rc;
    // ... then the rest of the layer on the B context rows: out-proj + residual, LN1, GELU(FFN1), FFN2 + residual, LN2
    if (int rc = layer_tail(w, ly, cw.ctx, cw.gin, TailSlots{cw.tmp, cw.h, nullptr, cw.ffn, cw.tmp}, cw.y, B, f.st)) return rc;
    return tap(n, cw.y, nullptr, B, 1);
}

// HF BertPooler on the CLS rows a forward wrote (src/evaluation/utils/models.py:350: model_out.pooler_output, the SimCSE baselines'
// rep): the checks here, the kernel in enc_pooler.hip.  The pooler's weights travel as plain arguments: aspire_bert_weights keeps
// its layout.
extern "C" int aspire_bert_pooler_f32(const float* cls, int64_t B, int64_t D, const float* w_pool, const float* b_pool, float* pooled,
                                      void* stream) {
    ASPIRE_REQUIRE(D == kD, ASPIRE_ERR_UNSUPPORTED, "hidden size %lld unsupported (the pooler is built for 768)", (long long)D);
    ASPIRE_REQUIRE(B >= 0, ASPIRE_ERR_INVALID_ARG, "negative row count %lld", (long long)B);
    if (B == 0) return ASPIRE_OK;
    ASPIRE_REQUIRE(cls && w_pool && b_pool && pooled, ASPIRE_ERR_INVALID_ARG, "null pointer");
    ASPIRE_REQUIRE(pooled != cls, ASPIRE_ERR_INVALID_ARG, "pooled must not be cls: a workgroup reads whole rows that others write");
    ASPIRE_REQUIRE(((uintptr_t)cls & 15) == 0 && ((uintptr_t)w_pool & 15) == 0, ASPIRE_ERR_INVALID_ARG,
                   "cls and w_pool must be 16-byte aligned");
    return launch_pooler(cls, B, w_pool, b_pool, pooled, (hipStream_t)stream);
}

// The _prec forwards' workspaces: the mode's H-layout activations live in the default path's P slots (twice their size), and a GEMM pin
// sends a forward of the mode down the default path, so both modes ask for the same bytes
extern "C" size_t aspire_bert_workspace_bytes_prec(const aspire_bert_weights* w, int64_t B, int64_t L, int matmul) {
    if (matmul != ASPIRE_MATMUL_FP32 && matmul != ASPIRE_MATMUL_FP16) return 0;
    return aspire_bert_workspace_bytes(w, B, L);
}
extern "C" size_t aspire_bert_cls_workspace_bytes_prec(const aspire_bert_weights* w, int64_t B, int64_t L, int matmul) {
    if (matmul != ASPIRE_MATMUL_FP32 && matmul != ASPIRE_MATMUL_FP16) return 0;
    return aspire_bert_cls_workspace_bytes(w, B, L);
}

// The weights' single fp16 planes of the fp16 matmul mode (the H layout, 64 w rounded once), formed ONCE when the model is loaded: a
// device buffer the caller keeps next to the weights and hands to the _prec forwards
extern "C" size_t aspire_bert_hplanes_bytes(const aspire_bert_weights* w) {
    if (!w || w->n_layers <= 0 || w->hidden != kD || w->ffn_dim <= 0) return 0;
    return hplane_offsets(w->ffn_dim).per_layer * (size_t)w->n_layers;
}

extern "C" int aspire_bert_prepare_hplanes(const aspire_bert_weights* w, void* hplanes, size_t hplanes_bytes, void* stream) {
    ASPIRE_REQUIRE(w && hplanes, ASPIRE_ERR_INVALID_ARG, "null pointer");
    ASPIRE_REQUIRE(w->hidden == kD && w->ffn_dim % 128 == 0 && w->ffn_dim > 0, ASPIRE_ERR_UNSUPPORTED,
                   "fp16 weight planes are built for hidden 768 and an ffn width that is a multiple of 128");
    ASPIRE_REQUIRE(w->n_layers > 0 && w->layers, ASPIRE_ERR_INVALID_ARG, "bad layer table");
    ASPIRE_REQUIRE(hplanes_bytes >= aspire_bert_hplanes_bytes(w), ASPIRE_ERR_INVALID_ARG, "hplanes buffer too small");
    if (int rc = check_layer_pointers(w->layers, w->n_layers, "weights")) return rc;
    hipStream_t st = (hipStream_t)stream;
    const PlaneOffsets ho = hplane_offsets(w->ffn_dim);
    int* too_big = nullptr;        // a load-time call: its own 4 bytes, one synchronisation at the end
    ASPIRE_HIP_OK(hipMalloc((void**)&too_big, sizeof(int)));
    int rc = ASPIRE_OK;
    auto split = [&](const float* X, int64_t R, int K, void* P) {
        if (rc == ASPIRE_OK) rc = launch_split_h(X, R, K, K, P, true, too_big, st);
    };
    hipError_t e0 = hipMemsetAsync(too_big, 0, sizeof(int), st);
    if (e0 == hipSuccess) e0 = hipMemsetAsync(hplanes, 0, aspire_bert_hplanes_bytes(w), st);      // the slack rows behind every matrix
    if (e0 != hipSuccess) {
        (void)hipFree(too_big);
        ASPIRE_HIP_OK(e0);
    }
    for (int l = 0; l < w->n_layers; ++l) {
        const aspire_bert_layer& ly = w->layers[l];
        char* lh = (char*)hplanes + (size_t)l * ho.per_layer;
        split(ly.w_qkv, 3 * kD, kD, lh + ho.qkv);
        split(ly.w_o, kD, kD, lh + ho.o);
        split(ly.w_ffn1, w->ffn_dim, kD, lh + ho.ffn1);
        split(ly.w_ffn2, kD, w->ffn_dim, lh + ho.ffn2);
    }
    int flag = 0;
    hipError_t e1 = rc == ASPIRE_OK ? hipMemcpyAsync(&flag, too_big, sizeof(int), hipMemcpyDeviceToHost, st) : hipSuccess;
    if (e1 == hipSuccess) e1 = hipStreamSynchronize(st);
    (void)hipFree(too_big);
    if (rc != ASPIRE_OK) return rc;
    ASPIRE_HIP_OK(e1);
    ASPIRE_REQUIRE(flag == 0, ASPIRE_ERR_UNSUPPORTED,
                   "a weight is not finite or beyond +-1023 (|64 w| > 65504): outside the fp16 matmul mode's range (run such a model with ASPIRE_MATMUL_FP32)");
    return ASPIRE_OK;
}

// The weights' fp16 planes, formed ONCE when the model is loaded: a device buffer of aspire_bert_planes_bytes(w) bytes that the
// caller keeps next to the weights and hands over as aspire_bert_weights::planes.
extern "C" size_t aspire_bert_planes_bytes(const aspire_bert_weights* w) {
    if (!w || w->n_layers <= 0 || w->hidden != kD || w->ffn_dim <= 0) return 0;
    return plane_offsets(w->ffn_dim).per_layer * (size_t)w->n_layers;
}

extern "C" int aspire_bert_prepare_planes(const aspire_bert_weights* w, void* planes, size_t planes_bytes, void* stream) {
    ASPIRE_REQUIRE(w && planes, ASPIRE_ERR_INVALID_ARG, "null pointer");
    ASPIRE_REQUIRE(w->hidden == kD && w->ffn_dim % 128 == 0 && w->ffn_dim > 0, ASPIRE_ERR_UNSUPPORTED,
                   "pre-split weights are built for hidden 768 and an ffn width that is a multiple of 128");
    ASPIRE_REQUIRE(planes_bytes >= aspire_bert_planes_bytes(w), ASPIRE_ERR_INVALID_ARG, "planes buffer too small");
    hipStream_t st = (hipStream_t)stream;
    const PlaneOffsets po = plane_offsets(w->ffn_dim);
    int* too_big = nullptr;        // a load-time call: its own 4 bytes, one synchronisation at the end
    ASPIRE_HIP_OK(hipMalloc((void**)&too_big, sizeof(int)));
    int rc = ASPIRE_OK;
    auto split = [&](const float* X, int64_t R, int K, void* P) {
        if (rc == ASPIRE_OK) rc = launch_split_planes(X, R, K, P, true, too_big, st);
    };
    hipError_t e0 = hipMemsetAsync(too_big, 0, sizeof(int), st);
    if (e0 == hipSuccess) e0 = hipMemsetAsync(planes, 0, aspire_bert_planes_bytes(w), st);      // the slack rows behind every matrix
    if (e0 != hipSuccess) {
        (void)hipFree(too_big);
        ASPIRE_HIP_OK(e0);
    }
    for (int l = 0; l < w->n_layers; ++l) {
        const aspire_bert_layer& ly = w->layers[l];
        char* lp = (char*)planes + (size_t)l * po.per_layer;
        split(ly.w_qkv, 3 * kD, kD, lp + po.qkv);
        split(ly.w_o, kD, kD, lp + po.o);
        split(ly.w_ffn1, w->ffn_dim, kD, lp + po.ffn1);
        split(ly.w_ffn2, kD, w->ffn_dim, lp + po.ffn2);
    }
    int flag = 0;
    hipError_t e1 = rc == ASPIRE_OK ? hipMemcpyAsync(&flag, too_big, sizeof(int), hipMemcpyDeviceToHost, st) : hipSuccess;
    if (e1 == hipSuccess) e1 = hipStreamSynchronize(st);
    (void)hipFree(too_big);
    if (rc != ASPIRE_OK) return rc;
    ASPIRE_HIP_OK(e1);
    ASPIRE_REQUIRE(flag == 0, ASPIRE_ERR_UNSUPPORTED,
                   "a weight is not finite or beyond +-1023: outside the fp16-plane GEMM's range (leave aspire_bert_weights::planes NULL for such a model)");
    return ASPIRE_OK;
}

// Tuning hooks (not part of include/aspire_hip.h): an operand into the P layout (weight != 0: the B side, scaled), and one C = A . B^T (+bias) GEMM on P operands
// (tools/gemmbench.py); swap != 0: the GELU -> P-layout epilogue (Cp [M, N]).
extern "C" size_t aspire_debug_planes_bytes(int64_t R, int64_t K) { return p_bytes(R, K); }
extern "C" int aspire_debug_split_planes(const float* X, int64_t R, int K, void* P, int weight, void* stream) {
    ASPIRE_REQUIRE(K % 32 == 0, ASPIRE_ERR_UNSUPPORTED, "K %% 32");
    return launch_split_planes(X, R, K, P, weight != 0, nullptr, (hipStream_t)stream);
}
extern "C" int aspire_debug_gemm_planes(const void* Ap, const void* Bp, float* C, void* Cp, const float* bias, int M, int N, int K, int swap,
                                        void* stream) {
    PGemmArgs pg{Ap, Bp, C, Cp, bias, nullptr, M, N, K, N, 0, 0};
    return launch_gemm_p(pg, swap != 0, (hipStream_t)stream);
}

// Tuning hook (not part of include/aspire_hip.h): one plain C = A . B^T (+bias) GEMM through the encoder's tile
// dispatch, for tools/gemmbench.py.  A [M,K], B [N,K], C [M,N], all row-major fp32 device pointers.
extern "C" int aspire_debug_gemm_f32(const float* A, const float* B, float* C, const float* bias, int M, int N, int K,
                                     void* stream) {
    return launch_gemm(linear(A, B, C, bias, nullptr, M, N, K), 1, false, (hipStream_t)stream);
}
