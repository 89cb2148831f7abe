// A1t: the BERT layer stack under training -- a forward that keeps what the backward needs on a caller-owned tape, and the backward from
// the gradient of last_hidden_state to every encoder parameter and to the embedding sum (HuggingFace BertModel, with its dropout
// when asked for; the table lookup in front of it stays the caller's).  fp32 accuracy throughout.
//
// Forward = the fp32-operand body that inference runs without planes, by the same functions (enc_host.h: linear, attention_gemm,
// layer_tail): launch_gemm with its bias / residual epilogues, the three-kernel attention (QK^T GEMM, softmax_mask_kernel, PV GEMM) and
// launch_layernorm -- neither the fp16-plane path nor the LayerNorm-in-the-epilogue exchange, so no kernel of a training step waits on
// another workgroup.  One difference, layer_tail's switch: the FFN1 GEMM runs with its GELU epilogue OFF and the activation is a pass of
// its own (gelu_forward_kernel, the same gelu_erf on the same fp32 value: the same bits), so that the pre-GELU value is what lands on the
// tape; GELU(u) itself is not kept, the backward forms it again.
//
// Tape (floats; every slot 256-byte aligned): [emb_sum M x 768] then per layer
//   x M x 768 (layer input) | qkv M x 2304 | P B x H x L x Lp (soft-max probabilities, pad columns zero) | ctx M x 768 |
//   s1 M x 768 (pre-LN1 sum) | h M x 768 (LN1 output) | u M x ffn (pre-GELU) | s2 M x 768 (pre-LN2 sum)
//
// Backward of layer l, y = LN2(s2), s2 = GELU(u) W2^T + b2 + h, u = h W1^T + b1, h = LN1(s1), s1 = ctx Wo^T + bo + x, last layer first:
//   ds2 = LN2'(dy [+ the residual branch's gradient])  -> dgamma2, dbeta2       layernorm_backward_kernel
//   db2 = colsum(ds2); dW2 = ds2^T . GELU(u) (TN); da = ds2 . W2 (B_KN); du = da GELU'(u); db1 = colsum(du); dW1 = du^T . h (TN)
//   dh = du . W1 (B_KN); ds1 = LN1'(dh + ds2) -> dgamma1, dbeta1; dbo = colsum(ds1); dWo = ds1^T . ctx (TN); dctx = ds1 . Wo (B_KN)
//   per (document, head): dV = P^T . dctx (TN); dP = dctx . V^T (nn.Linear form); dS = scale P (dP - sum dP P) in place;
//                         dQ = dS . K (B_KN); dK = dS^T . Q (TN)
//   dbqkv = colsum(dqkv); dWqkv = dqkv^T . x (TN); dx = dqkv . Wqkv (B_KN), and ds1 is the residual branch's gradient of the layer below
// and at the bottom the embedding LayerNorm's backward.  Every gradient buffer is written, none accumulated; no atomics.
//
// Dropout (the _dropout_ entry points; dropout_rng.h: the contract; enc_dropout.hip: the passes): s1 = drop(ctx Wo^T + bo) + x and
// s2 = drop(GELU(u) W2^T + b2) + h as a pass behind a GEMM without its residual epilogue, ctx = drop(P) V with the dropped P in the
// workspace's dprobs (the tape keeps P), x0 = drop(LN(emb)).  The backward forms each mask again: dz2 = keep . scale . ds2 -> d2 feeds
// db2 / dW2 / da, dz1 = keep . scale . ds1 -> d1 feeds dbo / dWo / dctx (ds2, ds1 themselves go down the residual), the dropped P is
// formed again in dprobs for dV, dP = keep . scale . (dctx V^T) in place, and keep . scale . (dy + dy_res) -> d1 stands in front of the
// embedding LayerNorm's backward.  A probability of 0 (or a NULL struct) launches none of this: the calls without dropout, bit for bit.
//
// The CLS read-out (aspire_bert_cls_mix_train_f32, aspire_bert_layers_backward_cls_f32; the bi-encoders' and sentence encoders' models):
// the CLS rows of the n_layers + 1 hidden states come off the tape's layer inputs and hidden_out, and their [B, 768] gradient is one more
// source of backward_stack -- mix[l] . grad_cls onto row (b, 0) of state l's gradient: the top gradient formed in d2, below it a B-row
// update of d3 behind backward_layer(l).  The in-batch cross-entropy of two towers' CLS rows has its entry points here as well; the
// kernels of both: enc_cls_train.hip.
//
// The matmul mode (the _prec_ entry points; ASPIRE_MATMUL_*): in ASPIRE_MATMUL_BF16 every product of both layer bodies -- the four
// projections, Q K^T and P V forward, the ten of the backward -- goes through launch_gemm_bf16 (enc_gemm_bf16.hip: operands rounded to
// bf16 once when staged, fp32 accumulators and epilogues); every other launch, the tape and the workspace are the same, in fp32.  In
// ASPIRE_MATMUL_FP32 launch_product (enc_host.h) launches what was launched before there was a mode.  In ASPIRE_MATMUL_BF16X3 the NT
// products are those same launches (gemm_bf16x3_kernel already), and the B_KN and TN products -- P V forward; da, dh, dctx, dx, dQ and
// every dW, dV, dK of the backward -- go through launch_gemm_bf16x3 (enc_gemm_bf16x3.hip: operands split into three bf16 planes when
// staged, six products per term, fp32 accumulators): fp32 accuracy on the bf16 matrix pipe.
//
// The attention form (the _attn_ entry points; ASPIRE_ATTENTION_*): with ASPIRE_ATTENTION_FLASH, which ASPIRE_MATMUL_BF16 alone takes,
// steps 2 - 4 of the forward are one launch (launch_flash_attn_train) that leaves the rows' (m, l) [B, H, L, 2] in the tape's P slot, and
// the backward's launches between dctx and the QKV projection's are launch_flash_attn_train_backward (D [B, H, L] in the workspace's dP
// slot): neither buffer has an L^2 term, so carve_tape and carve_train take the mode with the geometry and the _attn size queries
// answer for it.  ASPIRE_ATTENTION_GEMM: everything above, unchanged.
//
// Packed rows (the _packed entry points; include/aspire_hip.h: aspire_bert_packing): with ASPIRE_MATMUL_BF16 and ASPIRE_ATTENTION_FLASH
// the stack runs over the M = rows valid token rows alone.  Every row-wise launch above takes any M as it is; the entries gather
// emb_sum / grad_hidden into packed rows and scatter hidden_out / grad_emb_sum back to [B, L, 768] with zeros on masked rows
// (enc_pack.hip), the attention is the packed instantiation of the fused kernels, the hidden sites' dropout is keyed through row_src
// (the padded call's masks) and the CLS taps read each document's first packed row.  The tape is the flash tape with M = rows, the
// forward keeps its packed top state in the workspace's d1.
//
// This file is host only (the tape's and the workspace's carve, the two layer loops, the C entry points); the kernels: enc_bwd.hip (rows),
// enc_gemm.hip (launch_gemm, launch_gemm_tn), enc_gemm_bf16.hip (launch_gemm_bf16), enc_gemm_bf16x3.hip (launch_gemm_bf16x3), enc_attn.hip (launch_softmax_mask), enc_attn_train.hip (the fused training attention), enc_rows.hip
// (launch_layernorm).
#include <math.h>

#include "enc_host.h"

namespace aspire {
namespace {

struct Geometry {
    int64_t B, L, M;
    int Lp, H, dh, ffn, n_layers;
    size_t probs;     // floats of one layer's P; ASPIRE_ATTENTION_FLASH: of its row statistics (m, l) [B, H, L, 2]
    size_t dprobs;    // floats of the workspace's dP / dS; ASPIRE_ATTENTION_FLASH: of D [B, H, L]
    int attention;
    // the padding-free mode (the _packed entry points): M = the valid token rows, statistics [H, M, 2], D [H, M]
    bool packed = false;
    PackedDocs docs{};
    const int32_t* row_dst = nullptr;
    int max_len = 0;
    const int32_t* row_map() const { return packed ? docs.row_src : nullptr; }       // what keys the hidden sites' dropout
    ClsRows cls_rows() const { return ClsRows{docs.doc_start, docs.row_src, docs.rows, (int)(B * L)}; }
};
Geometry geometry(const aspire_bert_weights* w, int64_t B, int64_t L, int attention = ASPIRE_ATTENTION_GEMM) {
    Geometry g;
    g.B = B; g.L = L; g.M = B * L;
    g.Lp = (int)((L + 3) / 4 * 4);
    g.H = w->n_heads; g.dh = g.H > 0 ? kD / g.H : 0; g.ffn = w->ffn_dim; g.n_layers = w->n_layers > 0 ? w->n_layers : 0;
    g.attention = attention;
    const bool flash = attention == ASPIRE_ATTENTION_FLASH;
    g.probs = flash ? (size_t)B * g.H * L * 2 : (size_t)B * g.H * L * g.Lp;
    g.dprobs = flash ? (size_t)B * g.H * L : g.probs;
    return g;
}
// `rows` valid token rows of a [B, L] batch (docs may be all zero but for rows: the size queries)
Geometry geometry_packed(const aspire_bert_weights* w, int64_t B, int64_t L, const PackedDocs& docs, const int32_t* row_dst, int max_len) {
    Geometry g = geometry(w, B, L, ASPIRE_ATTENTION_FLASH);
    g.M = docs.rows;
    g.probs = (size_t)g.H * g.M * 2;
    g.dprobs = (size_t)g.H * g.M;
    g.packed = true; g.docs = docs; g.row_dst = row_dst; g.max_len = max_len;
    return g;
}

struct TapeLayer {
    float *x, *qkv, *probs, *ctx, *s1, *h, *u, *s2;
};
struct Tape {
    char* base;
    size_t emb_bytes, per_layer, total;
    size_t o_qkv, o_probs, o_ctx, o_s1, o_h, o_u, o_s2;
    float* emb() const { return (float*)base; }
    TapeLayer layer(int l) const {
        char* p = base + emb_bytes + (size_t)l * per_layer;
        return TapeLayer{(float*)p, (float*)(p + o_qkv), (float*)(p + o_probs), (float*)(p + o_ctx), (float*)(p + o_s1), (float*)(p + o_h),
                         (float*)(p + o_u), (float*)(p + o_s2)};
    }
};
Tape carve_tape(const void* base, const Geometry& g) {
    Tape t;
    t.base = (char*)base;
    const size_t row = (size_t)g.M * kD;
    Carver c(nullptr);              // offsets within one layer's slot; x sits at 0
    c.floats(row);
    t.o_qkv = c.off; c.floats(3 * row);
    t.o_probs = c.off; c.floats(g.probs);
    t.o_ctx = c.off; c.floats(row);
    t.o_s1 = c.off; c.floats(row);
    t.o_h = c.off; c.floats(row);
    t.o_u = c.off; c.floats((size_t)g.M * g.ffn);
    t.o_s2 = c.off; c.floats(row);
    t.per_layer = c.off;
    t.emb_bytes = align_up(row * sizeof(float));
    t.total = t.emb_bytes + (size_t)g.n_layers * t.per_layer;
    return t;
}

// one workspace for both calls: the forward uses `act` alone
struct TrainWorkspace {
    float *act, *big, *d1, *d2, *d3, *dqkv, *dprobs, *partial;      // GELU(u); da / du; ds2; a branch's dy; ds1; [dQ | dK | dV]; dP / dS; column-sum partials
    size_t total;
};
TrainWorkspace carve_train(void* base, const Geometry& g) {
    Carver c(base);
    TrainWorkspace w;
    const size_t M = (size_t)g.M;
    w.act = c.floats(M * g.ffn);
    w.big = c.floats(M * g.ffn);
    w.d1 = c.floats(M * kD);
    w.d2 = c.floats(M * kD);
    w.d3 = c.floats(M * kD);
    w.dqkv = c.floats(M * 3 * kD);
    w.dprobs = c.floats(g.dprobs);
    size_t part = layernorm_backward_partial_floats(g.M);
    const size_t c1 = colsum_partial_floats(g.M, 3 * kD), c2 = colsum_partial_floats(g.M, g.ffn > 0 ? g.ffn : 0);
    part = part > c1 ? part : c1;
    part = part > c2 ? part : c2;
    w.partial = c.floats(part);
    w.total = c.off;
    return w;
}

// what both calls check of the weights and the shape, before anything else is read
int check_train_args(const aspire_bert_weights* w, int64_t B, int64_t L) {
    if (int rc = check_bert_shape(w, B, L)) return rc;
    ASPIRE_REQUIRE(w->emb_ln_g && w->emb_ln_b, ASPIRE_ERR_INVALID_ARG, "null pointer (emb_ln_g / emb_ln_b)");
    if (int rc = check_layer_pointers(w->layers, w->n_layers, "weights")) return rc;
    // the GEMM arguments are ints and the column sums' row blocks a grid's y dimension
    const int wide = w->ffn_dim > 3 * kD ? w->ffn_dim : 3 * kD;
    ASPIRE_REQUIRE((double)B * (double)L * wide < 2147483648.0, ASPIRE_ERR_UNSUPPORTED,
                   "%lld token rows in one call: row x column indices are 32-bit (split the batch)", (long long)(B * L));
    return ASPIRE_OK;
}

// the caller's tape and workspace hold what the two size queries ask for
int check_train_buffers(const Geometry& q, const void* tape, size_t tape_bytes, const void* ws, size_t ws_bytes) {
    const size_t need_tape = carve_tape(nullptr, q).total, need_ws = carve_train(nullptr, q).total;
    ASPIRE_REQUIRE(tape && tape_bytes >= need_tape, ASPIRE_ERR_INVALID_ARG, "tape too small: need %zu bytes (aspire_bert_tape_bytes)", need_tape);
    ASPIRE_REQUIRE(ws && ws_bytes >= need_ws, ASPIRE_ERR_INVALID_ARG, "workspace too small: need %zu bytes (aspire_bert_train_workspace_bytes)",
                   need_ws);
    return ASPIRE_OK;
}

// dX [M, K] = dY [M, N] . W [N, K]: the contraction runs over W's rows -- the B_KN form
GemmArgs grad_input(const float* dY, const float* W, float* dX, int64_t M, int N, int K) {
    GemmArgs g{};
    g.A = dY; g.B = W; g.C = dX;
    g.M = (int)M; g.N = K; g.K = N; g.lda = N; g.ldb = K; g.ldc = K; g.nz2 = 1; g.alpha = 1.f;
    return g;
}
// dW [N, K] = dY [M, N]^T . X [M, K]: the TN form
GemmArgs grad_weight(const float* dY, const float* X, float* dW, int64_t M, int N, int K) {
    GemmArgs g{};
    g.A = dY; g.B = X; g.C = dW;
    g.M = N; g.N = K; g.K = (int)M; g.lda = N; g.ldb = K; g.ldc = K; g.nz2 = 1; g.alpha = 1.f;
    return g;
}

// The dropout of one call (dropout_rng.h).  A probability of 0 switches its sites off: they run exactly the launches of a call without
// dropout.
struct Dropout {
    float p_hidden = 0.f, p_attn = 0.f;
    uint64_t seed = 0;
    uint32_t step = 0;
    bool hidden() const { return p_hidden > 0.f; }
    bool attn() const { return p_attn > 0.f; }
    DropSite emb() const { return drop_site(seed, step, 0, p_hidden); }
    DropSite probs(int l) const { return drop_site(seed, step, 1 + 3 * (uint32_t)l, p_attn); }
    DropSite proj(int l) const { return drop_site(seed, step, 2 + 3 * (uint32_t)l, p_hidden); }
    DropSite ffn2(int l) const { return drop_site(seed, step, 3 + 3 * (uint32_t)l, p_hidden); }
};

int check_probability(float p, const char* name) {
    ASPIRE_REQUIRE(p >= 0.f && p < 1.f, ASPIRE_ERR_INVALID_ARG, "dropout probability %s = %g outside [0, 1)", name, (double)p);     // (NaN fails too)
    return ASPIRE_OK;
}
// the matmul mode of the _prec_ entry points (include/aspire_hip.h: ASPIRE_MATMUL_*)
int check_matmul(int matmul) {
    ASPIRE_REQUIRE(matmul == ASPIRE_MATMUL_FP32 || matmul == ASPIRE_MATMUL_BF16 || matmul == ASPIRE_MATMUL_BF16X3, ASPIRE_ERR_INVALID_ARG,
                   "matmul mode %d: ASPIRE_MATMUL_FP32 (0), ASPIRE_MATMUL_BF16 (1) or ASPIRE_MATMUL_BF16X3 (3)", matmul);
    return ASPIRE_OK;
}
// the attention form of the _attn_ entry points (include/aspire_hip.h: ASPIRE_ATTENTION_*): the fused form exists in bf16 alone
int check_attention(int attention, int matmul) {
    ASPIRE_REQUIRE(attention == ASPIRE_ATTENTION_GEMM || attention == ASPIRE_ATTENTION_FLASH, ASPIRE_ERR_INVALID_ARG,
                   "attention mode %d: ASPIRE_ATTENTION_GEMM (0) or ASPIRE_ATTENTION_FLASH (1)", attention);
    ASPIRE_REQUIRE(attention == ASPIRE_ATTENTION_GEMM || matmul == ASPIRE_MATMUL_BF16, ASPIRE_ERR_UNSUPPORTED,
                   "ASPIRE_ATTENTION_FLASH is built for ASPIRE_MATMUL_BF16 alone (matmul mode %d): a fused attention at fp32 accuracy does not exist",
                   matmul);
    return ASPIRE_OK;
}
int read_dropout(const aspire_bert_dropout* d, Dropout* out) {
    if (!d) return ASPIRE_OK;
    if (int rc = check_probability(d->p_hidden, "p_hidden")) return rc;
    if (int rc = check_probability(d->p_attn, "p_attn")) return rc;
    *out = Dropout{d->p_hidden, d->p_attn, d->seed, d->step};
    return ASPIRE_OK;
}

int forward_layer(const aspire_bert_weights* w, const Geometry& q, int l, const TapeLayer& t, const int64_t* mask, const TrainWorkspace& ws,
                  float* out, const Dropout& dr, int mm, hipStream_t st) {
    const aspire_bert_layer& ly = w->layers[l];
    float* act = ws.act;
    const DropSite probs = dr.probs(l), tail[2] = {dr.proj(l), dr.ffn2(l)};
    // 1. qkv = x . Wqkv^T + bqkv
    if (int rc = launch_product(mm, linear(t.x, ly.w_qkv, t.qkv, ly.b_qkv, nullptr, q.M, 3 * kD, kD), 1, kGemmNT, st)) return rc;
    // 2-4. the three-kernel attention; the masked soft-max runs in place: the tape's P
    // (with dropout the tape keeps the undropped P; the dropped copy the P.V product reads goes to the workspace's dprobs, free here)
    // (ASPIRE_ATTENTION_FLASH: one fused launch; the tape's slot keeps the rows' (m, l) instead of P)
    // (packed: the same kernels over the documents' own rows; no mask is read)
    if (q.packed) {
        if (int rc = launch_flash_attn_train_packed(t.qkv, q.docs, q.max_len, t.ctx, t.probs, q.B, q.H, dr.attn() ? &probs : nullptr, st)) return rc;
    } else if (q.attention == ASPIRE_ATTENTION_FLASH) {
        if (int rc = launch_flash_attn_train(t.qkv, mask, t.ctx, t.probs, q.B, (int)q.L, q.H, dr.attn() ? &probs : nullptr, st)) return rc;
    } else if (int rc = attention_gemm(t.qkv, t.probs, t.ctx, mask, q.B, q.L, q.Lp, q.H, q.dh, nullptr, 0, st, dr.attn() ? &probs : nullptr,
                                       ws.dprobs, mm))
        return rc;
    // 5. s1 = ctx . Wo^T + bo + x; h = LN1(s1)
    // 6. u = h . W1^T + b1 (GELU epilogue off); a = GELU(u); s2 = a . W2^T + b2 + h; out = LN2(s2)
    return layer_tail(w, ly, t.ctx, t.x, TailSlots{t.s1, t.h, t.u, act, t.s2}, out, q.M, st, dr.hidden() ? tail : nullptr, mm, q.row_map());
}

// the QKV projection's backward: ws.dqkv -> dbqkv, dWqkv and the gradient of the layer's input in ws.d2
int backward_qkv(const aspire_bert_weights* w, const Geometry& q, int l, const TapeLayer& t, const aspire_bert_layer_grads& gr,
                 const TrainWorkspace& ws, int mm, hipStream_t st) {
    const aspire_bert_layer& ly = w->layers[l];
    const int64_t M = q.M;
    if (int rc = launch_colsum(ws.dqkv, M, 3 * kD, gr.b_qkv, ws.partial, st)) return rc;
    if (int rc = launch_product(mm, grad_weight(ws.dqkv, t.x, gr.w_qkv, M, 3 * kD, kD), 1, kGemmTN, st)) return rc;
    return launch_product(mm, grad_input(ws.dqkv, ly.w_qkv, ws.d2, M, 3 * kD, kD), 1, kGemmBKN, st);
}

// dy (+ dy_res) = the gradient of layer l's output -> ws.d2 (+ ws.d3) = the gradient of its input, the layer's parameter gradients
int backward_layer(const aspire_bert_weights* w, const Geometry& q, int l, const TapeLayer& t, const aspire_bert_layer_grads& gr,
                   const float* dy, const float* dy_res, const TrainWorkspace& ws, const int64_t* mask, const Dropout& dr, int mm,
                   hipStream_t st) {
    const aspire_bert_layer& ly = w->layers[l];
    const int64_t M = q.M, L = q.L, B = q.B;
    const int H = q.H, dh = q.dh, Lp = q.Lp, ffn = q.ffn;
    const int batch = (int)(B * H);
    // LN2, FFN2
    if (int rc = launch_layernorm_backward(t.s2, ly.ln2_g, w->ln_eps, dy, dy_res, ws.d1, gr.ln2_g, gr.ln2_b, M, ws.partial, st)) return rc;
    // dropout: the FFN2 branch reads dz2 = keep . scale . ds2 (into d2: dy and dy_res, d2 / d3 below the top layer, are dead by now);
    // ds2 itself goes down the residual
    const float* dz2 = ws.d1;
    if (dr.hidden()) {
        if (int rc = launch_dropout_flat(ws.d1, nullptr, nullptr, ws.d2, M * kD, dr.ffn2(l), st, q.row_map())) return rc;
        dz2 = ws.d2;
    }
    if (int rc = launch_colsum(dz2, M, kD, gr.b_ffn2, ws.partial, st)) return rc;
    if (int rc = launch_gelu_forward(t.u, ws.act, M * ffn, st)) return rc;
    if (int rc = launch_product(mm, grad_weight(dz2, ws.act, gr.w_ffn2, M, kD, ffn), 1, kGemmTN, st)) return rc;
    if (int rc = launch_product(mm, grad_input(dz2, ly.w_ffn2, ws.big, M, kD, ffn), 1, kGemmBKN, st)) return rc;
    // GELU, FFN1
    if (int rc = launch_gelu_backward(ws.big, t.u, ws.big, M * ffn, st)) return rc;
    if (int rc = launch_colsum(ws.big, M, ffn, gr.b_ffn1, ws.partial, st)) return rc;
    if (int rc = launch_product(mm, grad_weight(ws.big, t.h, gr.w_ffn1, M, ffn, kD), 1, kGemmTN, st)) return rc;
    if (int rc = launch_product(mm, grad_input(ws.big, ly.w_ffn1, ws.d2, M, ffn, kD), 1, kGemmBKN, st)) return rc;
    // LN1 (dh = the FFN branch's gradient + ds2 down the residual), the output projection
    if (int rc = launch_layernorm_backward(t.s1, ly.ln1_g, w->ln_eps, ws.d2, ws.d1, ws.d3, gr.ln1_g, gr.ln1_b, M, ws.partial, st)) return rc;
    // dropout: the projection reads dz1 = keep . scale . ds1 (into d1: ds2 is dead once LN1's backward has read it); ds1 stays in d3,
    // the residual branch's gradient for the layer below
    const float* dz1 = ws.d3;
    if (dr.hidden()) {
        if (int rc = launch_dropout_flat(ws.d3, nullptr, nullptr, ws.d1, M * kD, dr.proj(l), st, q.row_map())) return rc;
        dz1 = ws.d1;
    }
    if (int rc = launch_colsum(dz1, M, kD, gr.b_o, ws.partial, st)) return rc;
    if (int rc = launch_product(mm, grad_weight(dz1, t.ctx, gr.w_o, M, kD, kD), 1, kGemmTN, st)) return rc;
    if (int rc = launch_product(mm, grad_input(dz1, ly.w_o, ws.d2, M, kD, kD), 1, kGemmBKN, st)) return rc;         // dctx
    // attention, per (document, head); dqkv = [dQ | dK | dV] in qkv's layout
    if (q.attention == ASPIRE_ATTENTION_FLASH) {
        // D = rowsum(dctx . ctx) into the workspace, then the key-block and the query-block kernels: every element of dqkv once
        const DropSite site = dr.probs(l);
        if (q.packed) {
            if (int rc = launch_flash_attn_train_backward_packed(t.qkv, q.docs, q.max_len, t.ctx, t.probs, ws.d2, ws.dprobs, ws.dqkv, B, H,
                                                                 dr.attn() ? &site : nullptr, st))
                return rc;
        } else if (int rc = launch_flash_attn_train_backward(t.qkv, mask, t.ctx, t.probs, ws.d2, ws.dprobs, ws.dqkv, B, (int)L, H,
                                                             dr.attn() ? &site : nullptr, st))
            return rc;
        return backward_qkv(w, q, l, t, gr, ws, mm, st);
    }
    const auto dP = prob_heads(ws.dprobs, H, L, Lp), dctx = ctx_heads(ws.d2, L, dh);
    const auto Q = qkv_heads(t.qkv, L, dh), K = qkv_heads(t.qkv + kD, L, dh), V = qkv_heads(t.qkv + 2 * kD, L, dh);
    const auto dQ = qkv_heads(ws.dqkv, L, dh), dK = qkv_heads(ws.dqkv + kD, L, dh), dV = qkv_heads(ws.dqkv + 2 * kD, L, dh);
    // dV_bh [keys, 64] = P_bh^T . dctx_bh; dropout: of the dropped P, formed again in dprobs (free until dP lands there)
    const DropSite drop_p = dr.probs(l);
    if (dr.attn())
        if (int rc = launch_dropout_probs(t.probs, ws.dprobs, B * H * L, (int)L, Lp, drop_p, st)) return rc;
    const auto P = prob_heads(dr.attn() ? ws.dprobs : t.probs, H, L, Lp);
    if (int rc = launch_product(mm, head_gemm(P, dctx, dV, L, dh, L, H), batch, kGemmTN, st)) return rc;
    // dP_bh [queries, keys] = dctx_bh . V_bh^T; dropout: that is the dropped P's gradient, the soft-max's is keep . scale . of it
    if (int rc = launch_product(mm, head_gemm(dctx, V, dP, L, L, dh, H), batch, kGemmNT, st)) return rc;
    if (dr.attn())
        if (int rc = launch_dropout_probs(ws.dprobs, ws.dprobs, B * H * L, (int)L, Lp, drop_p, st)) return rc;
    if (int rc = launch_softmax_backward(ws.dprobs, t.probs, B * H * L, (int)L, Lp, 1.0f / sqrtf((float)dh), st)) return rc;
    // dQ_bh = dS_bh . K_bh
    if (int rc = launch_product(mm, head_gemm(dP, K, dQ, L, dh, L, H), batch, kGemmBKN, st)) return rc;
    // dK_bh [keys, 64] = dS_bh^T . Q_bh
    if (int rc = launch_product(mm, head_gemm(dP, Q, dK, L, dh, L, H), batch, kGemmTN, st)) return rc;
    return backward_qkv(w, q, l, t, gr, ws, mm, st);
}

// The CLS read-out's gradient source (aspire_bert_layers_backward_cls_f32): row (b, 0) of hidden state l's gradient takes
// mix[l] . grad_cls[b, :] for every l, or with mix NULL the top state's alone, with factor 1
struct ClsSource {
    const float *grad_cls, *mix, *layer_cls;
    float* grad_mix;
};

// From the gradient of the top hidden state (grad_hidden, and / or the CLS rows of `cls`) to every parameter gradient and the embedding
// sum's.  cls NULL: the launches of the backward without a read-out source, none more.
int backward_stack(const aspire_bert_weights* w, const Geometry& q, const Tape& t, const TrainWorkspace& tw, const int64_t* mask,
                   const float* grad_hidden, const ClsSource* cls, float* grad_emb_sum, const aspire_bert_grads* grads, const Dropout& dr, int mm, hipStream_t st) {
    const float *dy = grad_hidden, *dy_res = nullptr;
    const ClsRows cls_rows = q.cls_rows();
    const ClsRows* packed_rows = q.packed ? &cls_rows : nullptr;
    if (q.packed && grad_hidden) {
        // the caller's gradient is padded: its valid rows, gathered into d2 (where the CLS source forms the top gradient as well); its
        // masked rows are never read
        if (int rc = launch_pack_rows(grad_hidden, q.docs.row_src, tw.d2, q.M, q.B * q.L, st)) return rc;
        dy = tw.d2;
    }
    if (cls) {
        // the top gradient = grad_hidden (or zeros) + the CLS rows, formed in d2: backward_layer writes d2 only after LN2's backward has
        // read dy, and the layers below hand their dy over in d2 as well
        const size_t bytes = (size_t)q.M * kD * sizeof(float);
        if (grad_hidden && !q.packed)
            ASPIRE_HIP_OK(hipMemcpyAsync(tw.d2, grad_hidden, bytes, hipMemcpyDeviceToDevice, st));
        else if (!grad_hidden)
            ASPIRE_HIP_OK(hipMemsetAsync(tw.d2, 0, bytes, st));
        if (int rc = launch_cls_inject(tw.d2, q.B, q.L, cls->grad_cls, cls->mix, q.n_layers, st, packed_rows)) return rc;
        dy = tw.d2;
        if (cls->grad_mix)
            if (int rc = launch_cls_grad_mix(cls->grad_cls, cls->layer_cls, q.B, q.n_layers + 1, cls->grad_mix, st)) return rc;
    }
    for (int l = q.n_layers - 1; l >= 0; --l) {
        if (int rc = backward_layer(w, q, l, t.layer(l), grads->layers[l], dy, dy_res, tw, mask, dr, mm, st)) return rc;
        dy = tw.d2;         // the attention branch's gradient of the layer's input ...
        dy_res = tw.d3;     // ... and ds1 down the residual: summed by the LayerNorm backward that reads them
        // hidden state l is this layer's input: its CLS rows' share of the mix lands on the residual branch's gradient, before the
        // LayerNorm backward below (or, for state 0, the backward of site 0's dropout) adds the two branches
        if (cls && cls->mix)
            if (int rc = launch_cls_inject(tw.d3, q.B, q.L, cls->grad_cls, cls->mix, l, st, packed_rows)) return rc;
    }
    // the embedding LayerNorm (grad_emb_sum NULL: its input gradient goes to scratch, the parameter gradients are still wanted)
    float* scratch = tw.d1;
    if (dr.hidden()) {
        // its output's gradient is keep . scale . (dy + dy_res), into d1; d2 is dead after that pass and takes the scratch's place
        if (int rc = launch_dropout_flat(dy, dy_res, nullptr, tw.d1, q.M * kD, dr.emb(), st, q.row_map())) return rc;
        dy = tw.d1; dy_res = nullptr; scratch = tw.d2;
    }
    if (q.packed) {
        // the packed rows' gradient into the scratch, then every padded row once: its packed row, or zeros
        if (int rc = launch_layernorm_backward(t.emb(), w->emb_ln_g, w->ln_eps, dy, dy_res, scratch, grads->emb_ln_g, grads->emb_ln_b, q.M,
                                               tw.partial, st))
            return rc;
        return grad_emb_sum ? launch_unpack_rows(scratch, q.row_dst, grad_emb_sum, q.B * q.L, q.M, st) : ASPIRE_OK;
    }
    return launch_layernorm_backward(t.emb(), w->emb_ln_g, w->ln_eps, dy, dy_res, grad_emb_sum ? grad_emb_sum : scratch, grads->emb_ln_g,
                                     grads->emb_ln_b, q.M, tw.partial, st);
}

// what the backward entry points share behind their own null checks: the dropout, geometry, gradient-table, tape and workspace checks,
// then the stack
int backward_entry(const aspire_bert_weights* w, const int64_t* mask, int64_t B, int64_t L, const float* grad_hidden, const ClsSource* cls, const void* tape,
                   size_t tape_bytes, float* grad_emb_sum, const aspire_bert_grads* grads, void* ws, size_t ws_bytes,
                   const aspire_bert_dropout* dropout, int matmul, int attention, void* stream) {
    if (int rc = check_matmul(matmul)) return rc;
    if (int rc = check_attention(attention, matmul)) return rc;
    Dropout dr;
    if (int rc = read_dropout(dropout, &dr)) return rc;
    if (int rc = check_train_args(w, B, L)) return rc;
    ASPIRE_REQUIRE(grads->emb_ln_g && grads->emb_ln_b && (w->n_layers == 0 || grads->layers), ASPIRE_ERR_INVALID_ARG,
                   "null pointer in the gradient table");
    if (int rc = check_layer_pointers(grads->layers, w->n_layers, "gradients")) return rc;
    if (B == 0) return ASPIRE_OK;
    const Geometry q = geometry(w, B, L, attention);
    if (int rc = check_train_buffers(q, tape, tape_bytes, ws, ws_bytes)) return rc;
    return backward_stack(w, q, carve_tape(tape, q), carve_train(ws, q), mask, grad_hidden, cls, grad_emb_sum, grads, dr, matmul, (hipStream_t)stream);
}

// the rows of the in-batch cross-entropy: both calls' checks
int check_xent_args(bool pointers, int64_t B, int64_t D) {
    ASPIRE_REQUIRE(B >= 0, ASPIRE_ERR_INVALID_ARG, "negative batch size %lld", (long long)B);
    ASPIRE_REQUIRE(D == kD, ASPIRE_ERR_UNSUPPORTED, "encoding dim %lld unsupported (kernels are built for 768)", (long long)D);
    ASPIRE_REQUIRE(B <= kXentMaxRows, ASPIRE_ERR_UNSUPPORTED, "%lld rows in one batch: the in-batch cross-entropy is built for at most %d",
                   (long long)B, kXentMaxRows);
    ASPIRE_REQUIRE(pointers, ASPIRE_ERR_INVALID_ARG, "null pointer");
    return ASPIRE_OK;
}
int check_xent_rows(const void* a, const void* b, const void* c = nullptr, const void* d = nullptr) {
    ASPIRE_REQUIRE((((uintptr_t)a | (uintptr_t)b | (uintptr_t)c | (uintptr_t)d) & 15) == 0, ASPIRE_ERR_INVALID_ARG,
                   "rows must be 16-byte aligned");
    return ASPIRE_OK;
}

}  // namespace
}  // namespace aspire

using namespace aspire;

extern "C" size_t aspire_bert_tape_bytes(const aspire_bert_weights* w, int64_t B, int64_t L) {
    if (!w || B <= 0 || L <= 0) return 0;
    return carve_tape(nullptr, geometry(w, B, L)).total;
}

extern "C" size_t aspire_bert_train_workspace_bytes(const aspire_bert_weights* w, int64_t B, int64_t L) {
    if (!w || B <= 0 || L <= 0) return 0;
    return carve_train(nullptr, geometry(w, B, L)).total;
}

extern "C" size_t aspire_bert_tape_bytes_attn(const aspire_bert_weights* w, int64_t B, int64_t L, int attention) {
    if (!w || B <= 0 || L <= 0 || (attention != ASPIRE_ATTENTION_GEMM && attention != ASPIRE_ATTENTION_FLASH)) return 0;
    return carve_tape(nullptr, geometry(w, B, L, attention)).total;
}

extern "C" size_t aspire_bert_train_workspace_bytes_attn(const aspire_bert_weights* w, int64_t B, int64_t L, int attention) {
    if (!w || B <= 0 || L <= 0 || (attention != ASPIRE_ATTENTION_GEMM && attention != ASPIRE_ATTENTION_FLASH)) return 0;
    return carve_train(nullptr, geometry(w, B, L, attention)).total;
}

extern "C" int aspire_bert_layers_forward_train_prec_f32(const aspire_bert_weights* w, const float* emb_sum, const int64_t* attn_mask,
                                                         int64_t B, int64_t L, float* hidden_out, void* tape, size_t tape_bytes, void* ws,
                                                         size_t ws_bytes, const aspire_bert_dropout* dropout, int matmul, void* stream) {
    return aspire_bert_layers_forward_train_attn_f32(w, emb_sum, attn_mask, B, L, hidden_out, tape, tape_bytes, ws, ws_bytes, dropout, matmul,
                                                     ASPIRE_ATTENTION_GEMM, stream);
}

extern "C" int aspire_bert_layers_forward_train_attn_f32(const aspire_bert_weights* w, const float* emb_sum, const int64_t* attn_mask,
                                                         int64_t B, int64_t L, float* hidden_out, void* tape, size_t tape_bytes, void* ws,
                                                         size_t ws_bytes, const aspire_bert_dropout* dropout, int matmul, int attention,
                                                         void* stream) {
    ASPIRE_REQUIRE(w && emb_sum && attn_mask && hidden_out, ASPIRE_ERR_INVALID_ARG, "null pointer");
    if (int rc = check_matmul(matmul)) return rc;
    if (int rc = check_attention(attention, matmul)) return rc;
    Dropout dr;
    if (int rc = read_dropout(dropout, &dr)) return rc;
    if (int rc = check_train_args(w, B, L)) return rc;
    if (B == 0) return ASPIRE_OK;
    const Geometry q = geometry(w, B, L, attention);
    if (int rc = check_train_buffers(q, tape, tape_bytes, ws, ws_bytes)) return rc;
    hipStream_t st = (hipStream_t)stream;
    const Tape t = carve_tape(tape, q);
    const TrainWorkspace tw = carve_train(ws, q);
    ASPIRE_HIP_OK(hipMemcpyAsync(t.emb(), emb_sum, (size_t)q.M * kD * sizeof(float), hipMemcpyDeviceToDevice, st));
    const int n = q.n_layers;
    float* x0 = n == 0 ? hidden_out : t.layer(0).x;
    if (int rc = launch_layernorm(t.emb(), w->emb_ln_g, w->emb_ln_b, w->ln_eps, x0, q.M, nullptr, st)) return rc;
    if (dr.hidden())
        if (int rc = launch_dropout_flat(x0, nullptr, nullptr, x0, q.M * kD, dr.emb(), st)) return rc;
    for (int l = 0; l < n; ++l)
        if (int rc = forward_layer(w, q, l, t.layer(l), attn_mask, tw, l == n - 1 ? hidden_out : t.layer(l + 1).x, dr, matmul, st))
            return rc;
    return ASPIRE_OK;
}

extern "C" int aspire_bert_layers_forward_train_dropout_f32(const aspire_bert_weights* w, const float* emb_sum, const int64_t* attn_mask,
                                                            int64_t B, int64_t L, float* hidden_out, void* tape, size_t tape_bytes, void* ws,
                                                            size_t ws_bytes, const aspire_bert_dropout* dropout, void* stream) {
    return aspire_bert_layers_forward_train_prec_f32(w, emb_sum, attn_mask, B, L, hidden_out, tape, tape_bytes, ws, ws_bytes, dropout,
                                                     ASPIRE_MATMUL_FP32, stream);
}

extern "C" int aspire_bert_layers_forward_train_f32(const aspire_bert_weights* w, const float* emb_sum, const int64_t* attn_mask, int64_t B,
                                                    int64_t L, float* hidden_out, void* tape, size_t tape_bytes, void* ws, size_t ws_bytes,
                                                    void* stream) {
    return aspire_bert_layers_forward_train_dropout_f32(w, emb_sum, attn_mask, B, L, hidden_out, tape, tape_bytes, ws, ws_bytes, nullptr, stream);
}

extern "C" int aspire_bert_layers_backward_dropout_f32(const aspire_bert_weights* w, const int64_t* attn_mask, int64_t B, int64_t L,
                                                       const float* grad_hidden, const void* tape, size_t tape_bytes, float* grad_emb_sum,
                                                       const aspire_bert_grads* grads, void* ws, size_t ws_bytes,
                                                       const aspire_bert_dropout* dropout, void* stream) {
    ASPIRE_REQUIRE(w && attn_mask && grad_hidden && grads, ASPIRE_ERR_INVALID_ARG, "null pointer");
    return backward_entry(w, attn_mask, B, L, grad_hidden, nullptr, tape, tape_bytes, grad_emb_sum, grads, ws, ws_bytes, dropout, ASPIRE_MATMUL_FP32,
                          ASPIRE_ATTENTION_GEMM, stream);
}

extern "C" int aspire_bert_layers_backward_f32(const aspire_bert_weights* w, const int64_t* attn_mask, int64_t B, int64_t L,
                                               const float* grad_hidden, const void* tape, size_t tape_bytes, float* grad_emb_sum,
                                               const aspire_bert_grads* grads, void* ws, size_t ws_bytes, void* stream) {
    return aspire_bert_layers_backward_dropout_f32(w, attn_mask, B, L, grad_hidden, tape, tape_bytes, grad_emb_sum, grads, ws, ws_bytes, nullptr,
                                                   stream);
}

extern "C" int aspire_bert_dropout_mask_u8(uint64_t seed, uint32_t step, int32_t site, float p, int64_t first, int64_t n,
                                           unsigned char* keep_out, void* stream) {
    if (int rc = check_probability(p, "p")) return rc;
    ASPIRE_REQUIRE(site >= 0 && first >= 0 && n >= 0, ASPIRE_ERR_INVALID_ARG, "negative site, first or n (%d, %lld, %lld)", (int)site,
                   (long long)first, (long long)n);
    ASPIRE_REQUIRE(keep_out, ASPIRE_ERR_INVALID_ARG, "null pointer (keep_out)");
    if (n == 0) return ASPIRE_OK;
    ASPIRE_REQUIRE(n < ((int64_t)1 << 39), ASPIRE_ERR_UNSUPPORTED, "%lld mask bytes in one call: the grid is 2^31 workgroups of 256", (long long)n);
    return launch_dropout_mask(keep_out, (uint64_t)first, n, drop_site(seed, step, (uint32_t)site, p), (hipStream_t)stream);
}

extern "C" int aspire_bert_cls_mix_train_f32(const aspire_bert_weights* w, int64_t B, int64_t L, const void* tape, size_t tape_bytes,
                                             const float* hidden_out, const float* mix, float* cls_out, float* layer_cls, void* stream) {
    return aspire_bert_cls_mix_train_attn_f32(w, B, L, tape, tape_bytes, hidden_out, mix, cls_out, layer_cls, ASPIRE_ATTENTION_GEMM, stream);
}

extern "C" int aspire_bert_cls_mix_train_attn_f32(const aspire_bert_weights* w, int64_t B, int64_t L, const void* tape, size_t tape_bytes,
                                                  const float* hidden_out, const float* mix, float* cls_out, float* layer_cls, int attention,
                                                  void* stream) {
    ASPIRE_REQUIRE(w && hidden_out && cls_out, ASPIRE_ERR_INVALID_ARG, "null pointer (w / hidden_out / cls_out)");
    ASPIRE_REQUIRE(!mix || layer_cls, ASPIRE_ERR_INVALID_ARG, "null pointer (layer_cls with a mix)");
    ASPIRE_REQUIRE(attention == ASPIRE_ATTENTION_GEMM || attention == ASPIRE_ATTENTION_FLASH, ASPIRE_ERR_INVALID_ARG,
                   "attention mode %d: ASPIRE_ATTENTION_GEMM (0) or ASPIRE_ATTENTION_FLASH (1)", attention);
    if (int rc = check_bert_shape(w, B, L)) return rc;
    if (B == 0) return ASPIRE_OK;
    const Geometry q = geometry(w, B, L, attention);
    const Tape t = carve_tape(tape, q);
    ASPIRE_REQUIRE(tape && tape_bytes >= t.total, ASPIRE_ERR_INVALID_ARG, "tape too small: need %zu bytes (aspire_bert_tape_bytes)", t.total);
    const ClsStates s{t.base + t.emb_bytes, t.per_layer, hidden_out, q.n_layers};
    return launch_cls_mix_tap(s, B, L, mix, cls_out, layer_cls, (hipStream_t)stream);
}

extern "C" int aspire_bert_layers_backward_prec_f32(const aspire_bert_weights* w, const int64_t* attn_mask, int64_t B, int64_t L,
                                                    const float* grad_hidden, const float* grad_cls, const float* mix, const float* layer_cls,
                                                    const void* tape, size_t tape_bytes, float* grad_emb_sum, const aspire_bert_grads* grads,
                                                    float* grad_mix, void* ws, size_t ws_bytes, const aspire_bert_dropout* dropout,
                                                    int matmul, void* stream) {
    return aspire_bert_layers_backward_attn_f32(w, attn_mask, B, L, grad_hidden, grad_cls, mix, layer_cls, tape, tape_bytes, grad_emb_sum, grads,
                                                grad_mix, ws, ws_bytes, dropout, matmul, ASPIRE_ATTENTION_GEMM, stream);
}

extern "C" int aspire_bert_layers_backward_attn_f32(const aspire_bert_weights* w, const int64_t* attn_mask, int64_t B, int64_t L,
                                                    const float* grad_hidden, const float* grad_cls, const float* mix, const float* layer_cls,
                                                    const void* tape, size_t tape_bytes, float* grad_emb_sum, const aspire_bert_grads* grads,
                                                    float* grad_mix, void* ws, size_t ws_bytes, const aspire_bert_dropout* dropout,
                                                    int matmul, int attention, void* stream) {
    ASPIRE_REQUIRE(w && attn_mask && grads, ASPIRE_ERR_INVALID_ARG, "null pointer");
    ASPIRE_REQUIRE(grad_hidden || grad_cls, ASPIRE_ERR_INVALID_ARG, "null pointer (grad_hidden and grad_cls: no gradient source)");
    ASPIRE_REQUIRE(!grad_mix || (layer_cls && mix && grad_cls), ASPIRE_ERR_INVALID_ARG,
                   "grad_mix needs grad_cls, mix and layer_cls (null pointer)");
    const ClsSource cls{grad_cls, mix, layer_cls, grad_mix};
    return backward_entry(w, attn_mask, B, L, grad_hidden, grad_cls ? &cls : nullptr, tape, tape_bytes, grad_emb_sum, grads, ws, ws_bytes, dropout,
                          matmul, attention, stream);
}

// ---- the padding-free mode: the stack over the valid token rows alone (include/aspire_hip.h: aspire_bert_packing) ----------------------
namespace {
// what the packed calls check before anything is read: the modes, the weights and the shape, the packing; -> the call's geometry
int packed_geometry(const aspire_bert_weights* w, const aspire_bert_packing* packing, int64_t B, int64_t L, int matmul, int attention,
                    Geometry* out) {
    if (int rc = check_matmul(matmul)) return rc;
    if (int rc = check_attention(attention, matmul)) return rc;
    ASPIRE_REQUIRE(attention == ASPIRE_ATTENTION_FLASH, ASPIRE_ERR_UNSUPPORTED,
                   "packed rows are built for ASPIRE_ATTENTION_FLASH alone (attention mode %d): the three-kernel attention has per-document "
                   "[L, L] matrices",
                   attention);
    if (int rc = check_bert_shape(w, B, L)) return rc;
    ASPIRE_REQUIRE(w->emb_ln_g && w->emb_ln_b, ASPIRE_ERR_INVALID_ARG, "null pointer (emb_ln_g / emb_ln_b)");
    if (int rc = check_layer_pointers(w->layers, w->n_layers, "weights")) return rc;
    PackedDocs docs{};
    if (int rc = read_packing(packing, B, L, &docs)) return rc;
    const int wide = w->ffn_dim > 3 * kD ? w->ffn_dim : 3 * kD;
    ASPIRE_REQUIRE((double)docs.rows * wide < 2147483648.0, ASPIRE_ERR_UNSUPPORTED,
                   "%d token rows in one call: row x column indices are 32-bit (split the batch)", docs.rows);
    *out = geometry_packed(w, B, L, docs, packing->row_dst, (int)packing->max_len);
    return ASPIRE_OK;
}
int check_packed_buffers(const Geometry& q, const void* tape, size_t tape_bytes, const void* ws, size_t ws_bytes) {
    const size_t need_tape = carve_tape(nullptr, q).total, need_ws = carve_train(nullptr, q).total;
    ASPIRE_REQUIRE(tape && tape_bytes >= need_tape, ASPIRE_ERR_INVALID_ARG, "tape too small: need %zu bytes (aspire_bert_tape_bytes_packed)",
                   need_tape);
    ASPIRE_REQUIRE(ws && ws_bytes >= need_ws, ASPIRE_ERR_INVALID_ARG,
                   "workspace too small: need %zu bytes (aspire_bert_train_workspace_bytes_packed)", need_ws);
    return ASPIRE_OK;
}
Geometry size_geometry(const aspire_bert_weights* w, int64_t B, int64_t L, int64_t rows) {
    PackedDocs docs{};
    docs.rows = (int)rows;
    return geometry_packed(w, B, L, docs, nullptr, 0);
}
bool packed_size_args(const aspire_bert_weights* w, int64_t B, int64_t L, int64_t rows) {
    return w && B > 0 && L > 0 && rows > 0 && (double)B * (double)L < 2147483648.0 && rows <= B * L;
}
// no valid row: every gradient is an exact zero (memory sets, no launch)
int zero_gradients(const aspire_bert_weights* w, const aspire_bert_grads* g, float* grad_emb_sum, float* grad_mix, int64_t B, int64_t L,
                   hipStream_t st) {
    const size_t f = sizeof(float), ffn = (size_t)w->ffn_dim;
    ASPIRE_HIP_OK(hipMemsetAsync(g->emb_ln_g, 0, kD * f, st));
    ASPIRE_HIP_OK(hipMemsetAsync(g->emb_ln_b, 0, kD * f, st));
    for (int l = 0; l < w->n_layers; ++l) {
        const aspire_bert_layer_grads& y = g->layers[l];
        float* const ptr[12] = {y.w_qkv, y.b_qkv, y.w_o, y.b_o, y.ln1_g, y.ln1_b, y.w_ffn1, y.b_ffn1, y.w_ffn2, y.b_ffn2, y.ln2_g, y.ln2_b};
        const size_t n[12] = {(size_t)3 * kD * kD, (size_t)3 * kD, (size_t)kD * kD, kD, kD, kD, ffn * kD, ffn, ffn * kD, kD, kD, kD};
        for (int i = 0; i < 12; ++i) ASPIRE_HIP_OK(hipMemsetAsync(ptr[i], 0, n[i] * f, st));
    }
    if (grad_emb_sum) ASPIRE_HIP_OK(hipMemsetAsync(grad_emb_sum, 0, (size_t)B * L * kD * f, st));
    if (grad_mix) ASPIRE_HIP_OK(hipMemsetAsync(grad_mix, 0, (size_t)(w->n_layers + 1) * f, st));
    return ASPIRE_OK;
}
}  // namespace

extern "C" size_t aspire_bert_tape_bytes_packed(const aspire_bert_weights* w, int64_t B, int64_t L, int64_t rows) {
    if (!packed_size_args(w, B, L, rows)) return 0;
    return carve_tape(nullptr, size_geometry(w, B, L, rows)).total;
}

extern "C" size_t aspire_bert_train_workspace_bytes_packed(const aspire_bert_weights* w, int64_t B, int64_t L, int64_t rows) {
    if (!packed_size_args(w, B, L, rows)) return 0;
    return carve_train(nullptr, size_geometry(w, B, L, rows)).total;
}

extern "C" int aspire_bert_layers_forward_train_packed_f32(const aspire_bert_weights* w, const float* emb_sum,
                                                           const aspire_bert_packing* packing, int64_t B, int64_t L, float* hidden_out,
                                                           void* tape, size_t tape_bytes, void* ws, size_t ws_bytes,
                                                           const aspire_bert_dropout* dropout, int matmul, int attention, void* stream) {
    ASPIRE_REQUIRE(w && emb_sum && packing && hidden_out, ASPIRE_ERR_INVALID_ARG, "null pointer");
    Dropout dr;
    if (int rc = read_dropout(dropout, &dr)) return rc;
    Geometry q;
    if (int rc = packed_geometry(w, packing, B, L, matmul, attention, &q)) return rc;
    if (B == 0) return ASPIRE_OK;
    hipStream_t st = (hipStream_t)stream;
    if (q.M == 0) {       // no valid token: zeros, no launch
        ASPIRE_HIP_OK(hipMemsetAsync(hidden_out, 0, (size_t)B * L * kD * sizeof(float), st));
        return ASPIRE_OK;
    }
    if (int rc = check_packed_buffers(q, tape, tape_bytes, ws, ws_bytes)) return rc;
    const Tape t = carve_tape(tape, q);
    const TrainWorkspace tw = carve_train(ws, q);
    if (int rc = launch_pack_rows(emb_sum, q.docs.row_src, t.emb(), q.M, B * L, st)) return rc;
    const int n = q.n_layers;
    float* top = tw.d1;                    // the packed top state: the forward uses act alone of the workspace
    float* x0 = n == 0 ? top : t.layer(0).x;
    if (int rc = launch_layernorm(t.emb(), w->emb_ln_g, w->emb_ln_b, w->ln_eps, x0, q.M, nullptr, st)) return rc;
    if (dr.hidden())
        if (int rc = launch_dropout_flat(x0, nullptr, nullptr, x0, q.M * kD, dr.emb(), st, q.row_map())) return rc;
    for (int l = 0; l < n; ++l)
        if (int rc = forward_layer(w, q, l, t.layer(l), nullptr, tw, l == n - 1 ? top : t.layer(l + 1).x, dr, matmul, st)) return rc;
    return launch_unpack_rows(top, q.row_dst, hidden_out, B * L, q.M, st);
}

extern "C" int aspire_bert_layers_backward_packed_f32(const aspire_bert_weights* w, const aspire_bert_packing* packing, int64_t B, int64_t L,
                                                      const float* grad_hidden, const float* grad_cls, const float* mix,
                                                      const float* layer_cls, const void* tape, size_t tape_bytes, float* grad_emb_sum,
                                                      const aspire_bert_grads* grads, float* grad_mix, void* ws, size_t ws_bytes,
                                                      const aspire_bert_dropout* dropout, int matmul, int attention, void* stream) {
    ASPIRE_REQUIRE(w && packing && grads, ASPIRE_ERR_INVALID_ARG, "null pointer");
    ASPIRE_REQUIRE(grad_hidden || grad_cls, ASPIRE_ERR_INVALID_ARG, "null pointer (grad_hidden and grad_cls: no gradient source)");
    ASPIRE_REQUIRE(!grad_mix || (layer_cls && mix && grad_cls), ASPIRE_ERR_INVALID_ARG,
                   "grad_mix needs grad_cls, mix and layer_cls (null pointer)");
    Dropout dr;
    if (int rc = read_dropout(dropout, &dr)) return rc;
    Geometry q;
    if (int rc = packed_geometry(w, packing, B, L, matmul, attention, &q)) return rc;
    ASPIRE_REQUIRE(grads->emb_ln_g && grads->emb_ln_b && (w->n_layers == 0 || grads->layers), ASPIRE_ERR_INVALID_ARG,
                   "null pointer in the gradient table");
    if (int rc = check_layer_pointers(grads->layers, w->n_layers, "gradients")) return rc;
    if (B == 0) return ASPIRE_OK;
    if (q.M == 0) return zero_gradients(w, grads, grad_emb_sum, grad_mix, B, L, (hipStream_t)stream);
    if (int rc = check_packed_buffers(q, tape, tape_bytes, ws, ws_bytes)) return rc;
    const ClsSource cls{grad_cls, mix, layer_cls, grad_mix};
    return backward_stack(w, q, carve_tape(tape, q), carve_train(ws, q), nullptr, grad_hidden, grad_cls ? &cls : nullptr, grad_emb_sum, grads, dr,
                          matmul, (hipStream_t)stream);
}

extern "C" int aspire_bert_cls_mix_train_packed_f32(const aspire_bert_weights* w, const aspire_bert_packing* packing, int64_t B, int64_t L,
                                                    const void* tape, size_t tape_bytes, const float* hidden_out, const float* mix,
                                                    float* cls_out, float* layer_cls, void* stream) {
    ASPIRE_REQUIRE(w && packing && hidden_out && cls_out, ASPIRE_ERR_INVALID_ARG, "null pointer (w / packing / hidden_out / cls_out)");
    ASPIRE_REQUIRE(!mix || layer_cls, ASPIRE_ERR_INVALID_ARG, "null pointer (layer_cls with a mix)");
    if (int rc = check_bert_shape(w, B, L)) return rc;
    PackedDocs docs{};
    if (int rc = read_packing(packing, B, L, &docs)) return rc;
    if (B == 0) return ASPIRE_OK;
    // every document's CLS row is its first packed row: a document without rows has none (the caller checks mask[:, 0] on the host)
    ASPIRE_REQUIRE(docs.rows >= B, ASPIRE_ERR_INVALID_ARG, "packing: %d rows for %lld documents -- a document without a CLS row", docs.rows,
                   (long long)B);
    const Geometry q = geometry_packed(w, B, L, docs, packing->row_dst, (int)packing->max_len);
    const Tape t = carve_tape(tape, q);
    ASPIRE_REQUIRE(tape && tape_bytes >= t.total, ASPIRE_ERR_INVALID_ARG, "tape too small: need %zu bytes (aspire_bert_tape_bytes_packed)", t.total);
    const ClsStates s{t.base + t.emb_bytes, t.per_layer, hidden_out, q.n_layers};
    const ClsRows rows = q.cls_rows();
    return launch_cls_mix_tap(s, B, L, mix, cls_out, layer_cls, (hipStream_t)stream, &rows);
}

extern "C" int aspire_bert_layers_backward_cls_f32(const aspire_bert_weights* w, const int64_t* attn_mask, int64_t B, int64_t L,
                                                   const float* grad_hidden, const float* grad_cls, const float* mix, const float* layer_cls,
                                                   const void* tape, size_t tape_bytes, float* grad_emb_sum, const aspire_bert_grads* grads,
                                                   float* grad_mix, void* ws, size_t ws_bytes, const aspire_bert_dropout* dropout,
                                                   void* stream) {
    return aspire_bert_layers_backward_prec_f32(w, attn_mask, B, L, grad_hidden, grad_cls, mix, layer_cls, tape, tape_bytes, grad_emb_sum, grads,
                                                grad_mix, ws, ws_bytes, dropout, ASPIRE_MATMUL_FP32, stream);
}

extern "C" int aspire_inbatch_xent_f32(const float* q, const float* c, int64_t B, int64_t D, float* loss, float* row_lse, void* stream) {
    if (int rc = check_xent_args(q && c && loss && row_lse, B, D)) return rc;
    if (B == 0) return ASPIRE_OK;
    if (int rc = check_xent_rows(q, c)) return rc;
    return launch_inbatch_xent(q, c, (int)B, loss, row_lse, (hipStream_t)stream);
}

extern "C" int aspire_inbatch_xent_backward_f32(const float* q, const float* c, int64_t B, int64_t D, const float* row_lse,
                                                const float* grad_loss, float* grad_q, float* grad_c, void* stream) {
    if (int rc = check_xent_args(q && c && row_lse && grad_loss && grad_q && grad_c, B, D)) return rc;
    if (B == 0) return ASPIRE_OK;
    if (int rc = check_xent_rows(q, c, grad_q, grad_c)) return rc;
    return launch_inbatch_xent_backward(q, c, (int)B, grad_loss, grad_q, grad_c, (hipStream_t)stream);
}
