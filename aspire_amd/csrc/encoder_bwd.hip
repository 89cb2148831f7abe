// A1t: the BERT layer stack under training -- a forward that keeps what the backward needs on a caller-owned tape, and the backward from
// the gradient of last_hidden_state to every encoder parameter and to the embedding sum (HuggingFace BertModel with both dropout
// probabilities 0; the table lookup in front of it stays the caller's).  fp32 accuracy throughout.
//
// Forward = the fp32-operand path of run_layer (encoder.hip), launch for launch: launch_gemm with its bias / residual epilogues, the
// three-kernel attention (QK^T GEMM, softmax_mask_kernel, PV GEMM) and launch_layernorm -- neither the fp16-plane path nor the
// LayerNorm-in-the-epilogue exchange, so no kernel of a training step waits on another workgroup.  One difference: the FFN1 GEMM runs
// with its GELU epilogue OFF and the activation is a pass of its own (gelu_forward_kernel, the same gelu_erf on the same fp32 value: the
// same bits), so that the pre-GELU value is what lands on the tape; GELU(u) itself is not kept, the backward forms it again.
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
// This file is host only (the tape's and the workspace's carve, the two layer loops, the C entry points); the kernels: enc_bwd.hip (rows),
// enc_gemm.hip (launch_gemm, launch_gemm_tn), enc_attn.hip (launch_softmax_mask), enc_rows.hip (launch_layernorm).
#include <math.h>

#include "enc_types.h"

namespace aspire {
namespace {

size_t align_up(size_t x) { return (x + 255) & ~(size_t)255; }

struct Geometry {
    int64_t B, L, M;
    int Lp, H, dh, ffn, n_layers;
    size_t probs;     // floats of one layer's P
};
Geometry geometry(const aspire_bert_weights* w, int64_t B, int64_t L) {
    Geometry g;
    g.B = B; g.L = L; g.M = B * L;
    g.Lp = (int)((L + 3) / 4 * 4);
    g.H = w->n_heads; g.dh = g.H > 0 ? kD / g.H : 0; g.ffn = w->ffn_dim; g.n_layers = w->n_layers > 0 ? w->n_layers : 0;
    g.probs = (size_t)B * g.H * L * g.Lp;
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
    const size_t row = align_up((size_t)g.M * kD * sizeof(float));
    t.emb_bytes = row;
    size_t off = row;                                                      // x
    t.o_qkv = off; off += align_up((size_t)g.M * 3 * kD * sizeof(float));
    t.o_probs = off; off += align_up(g.probs * sizeof(float));
    t.o_ctx = off; off += row;
    t.o_s1 = off; off += row;
    t.o_h = off; off += row;
    t.o_u = off; off += align_up((size_t)g.M * g.ffn * sizeof(float));
    t.o_s2 = off; off += row;
    t.per_layer = off;
    t.total = t.emb_bytes + (size_t)g.n_layers * t.per_layer;
    return t;
}

// one workspace for both calls: the forward uses `act` alone
struct TrainWorkspace {
    float *act, *big, *d1, *d2, *d3, *dqkv, *dprobs, *partial;      // GELU(u); da / du; ds2; a branch's dy; ds1; [dQ | dK | dV]; dP / dS; column-sum partials
    size_t total;
};
TrainWorkspace carve_train(void* base, const Geometry& g) {
    char* p = (char*)base;
    TrainWorkspace w;
    size_t off = 0;
    auto take = [&](size_t nfloats) {
        float* r = (float*)(p + off);
        off += align_up(nfloats * sizeof(float));
        return r;
    };
    const size_t M = (size_t)g.M;
    w.act = take(M * g.ffn);
    w.big = take(M * g.ffn);
    w.d1 = take(M * kD);
    w.d2 = take(M * kD);
    w.d3 = take(M * kD);
    w.dqkv = take(M * 3 * kD);
    w.dprobs = take(g.probs);
    size_t part = layernorm_backward_partial_floats(g.M);
    const size_t c1 = colsum_partial_floats(g.M, 3 * kD), c2 = colsum_partial_floats(g.M, g.ffn > 0 ? g.ffn : 0);
    part = part > c1 ? part : c1;
    part = part > c2 ? part : c2;
    w.partial = take(part);
    w.total = off;
    return w;
}

// what both calls check of the weights and the shape, before anything else is read
int check_train_args(const aspire_bert_weights* w, int64_t B, int64_t L) {
    ASPIRE_REQUIRE(w->hidden == kD && w->n_heads == 12 && w->ffn_dim % 64 == 0 && w->ffn_dim > 0, ASPIRE_ERR_UNSUPPORTED,
                   "only BERT-base geometry is built (hidden 768, 12 heads, ffn_dim %% 64 == 0); got hidden %d heads %d ffn_dim %d", w->hidden,
                   w->n_heads, w->ffn_dim);
    ASPIRE_REQUIRE(B >= 0 && L > 0 && L <= 512, ASPIRE_ERR_INVALID_ARG, "sequence length %lld outside (0, 512] (or a negative batch size)",
                   (long long)L);
    ASPIRE_REQUIRE(w->n_layers >= 0 && (w->n_layers == 0 || w->layers), ASPIRE_ERR_INVALID_ARG, "bad layer table");
    ASPIRE_REQUIRE(w->emb_ln_g && w->emb_ln_b, ASPIRE_ERR_INVALID_ARG, "null pointer (emb_ln_g / emb_ln_b)");
    for (int l = 0; l < w->n_layers; ++l) {
        const aspire_bert_layer& y = w->layers[l];
        ASPIRE_REQUIRE(y.w_qkv && y.b_qkv && y.w_o && y.b_o && y.ln1_g && y.ln1_b && y.w_ffn1 && y.b_ffn1 && y.w_ffn2 && y.b_ffn2 && y.ln2_g &&
                           y.ln2_b,
                       ASPIRE_ERR_INVALID_ARG, "null pointer in layer %d's weights", l);
    }
    // the GEMM arguments are ints and the column sums' row blocks a grid's y dimension
    const int wide = w->ffn_dim > 3 * kD ? w->ffn_dim : 3 * kD;
    ASPIRE_REQUIRE((double)B * (double)L * wide < 2147483648.0, ASPIRE_ERR_UNSUPPORTED,
                   "%lld token rows in one call: row x column indices are 32-bit (split the batch)", (long long)(B * L));
    return ASPIRE_OK;
}

GemmArgs linear(const float* A, const float* W, float* C, const float* bias, const float* res, int64_t M, int N, int K) {
    GemmArgs g{};
    g.A = A; g.B = W; g.C = C; g.bias = bias; g.res = res; g.ldr = N;
    g.M = (int)M; g.N = N; g.K = K; g.lda = K; g.ldb = K; g.ldc = N; g.nz2 = 1; g.alpha = 1.f;
    return g;
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

int forward_layer(const aspire_bert_weights* w, const Geometry& q, int l, const TapeLayer& t, const int64_t* mask, float* act, float* out,
                  hipStream_t st) {
    const aspire_bert_layer& ly = w->layers[l];
    const int64_t M = q.M, L = q.L, B = q.B;
    const int H = q.H, dh = q.dh, Lp = q.Lp, ffn = q.ffn;
    // 1. qkv = x . Wqkv^T + bqkv
    if (int rc = launch_gemm(linear(t.x, ly.w_qkv, t.qkv, ly.b_qkv, nullptr, M, 3 * kD, kD), 1, false, st)) return rc;
    // 2. scores[b, h] = Q_bh . K_bh^T
    GemmArgs g{};
    g.A = t.qkv; g.B = t.qkv + kD; g.C = t.probs;
    g.M = (int)L; g.N = (int)L; g.K = dh; g.lda = 3 * kD; g.ldb = 3 * kD; g.ldc = Lp; g.nz2 = H; g.alpha = 1.f;
    g.sa1 = (long long)L * 3 * kD; g.sa2 = dh; g.sb1 = g.sa1; g.sb2 = dh;
    g.sc1 = (long long)H * L * Lp; g.sc2 = (long long)L * Lp;
    if (int rc = launch_gemm(g, (int)(B * H), false, st)) return rc;
    // 3. the masked soft-max, in place: the tape's P
    if (int rc = launch_softmax_mask(t.probs, mask, B * H * L, (int)L, Lp, (int)(H * L), 1.0f / sqrtf((float)dh), nullptr, 0, st)) return rc;
    // 4. ctx[b, :, h] = P_bh . V_bh
    g = GemmArgs{};
    g.A = t.probs; g.B = t.qkv + 2 * kD; g.C = t.ctx;
    g.M = (int)L; g.N = dh; g.K = (int)L; g.lda = Lp; g.ldb = 3 * kD; g.ldc = kD; g.nz2 = H; g.alpha = 1.f;
    g.sa1 = (long long)H * L * Lp; g.sa2 = (long long)L * Lp; g.sb1 = (long long)L * 3 * kD; g.sb2 = dh;
    g.sc1 = (long long)L * kD; g.sc2 = dh;
    if (int rc = launch_gemm(g, (int)(B * H), true, st)) return rc;
    // 5. s1 = ctx . Wo^T + bo + x; h = LN1(s1)
    if (int rc = launch_gemm(linear(t.ctx, ly.w_o, t.s1, ly.b_o, t.x, M, kD, kD), 1, false, st)) return rc;
    if (int rc = launch_layernorm(t.s1, ly.ln1_g, ly.ln1_b, w->ln_eps, t.h, M, nullptr, st)) return rc;
    // 6. u = h . W1^T + b1 (GELU epilogue off); a = GELU(u); s2 = a . W2^T + b2 + h; out = LN2(s2)
    if (int rc = launch_gemm(linear(t.h, ly.w_ffn1, t.u, ly.b_ffn1, nullptr, M, ffn, kD), 1, false, st)) return rc;
    if (int rc = launch_gelu_forward(t.u, act, M * ffn, st)) return rc;
    if (int rc = launch_gemm(linear(act, ly.w_ffn2, t.s2, ly.b_ffn2, t.h, M, kD, ffn), 1, false, st)) return rc;
    return launch_layernorm(t.s2, ly.ln2_g, ly.ln2_b, w->ln_eps, out, M, nullptr, st);
}

// dy (+ dy_res) = the gradient of layer l's output -> ws.d2 (+ ws.d3) = the gradient of its input, the layer's parameter gradients
int backward_layer(const aspire_bert_weights* w, const Geometry& q, int l, const TapeLayer& t, const aspire_bert_layer_grads& gr,
                   const float* dy, const float* dy_res, const TrainWorkspace& ws, hipStream_t st) {
    const aspire_bert_layer& ly = w->layers[l];
    const int64_t M = q.M, L = q.L, B = q.B;
    const int H = q.H, dh = q.dh, Lp = q.Lp, ffn = q.ffn;
    const int batch = (int)(B * H);
    // LN2, FFN2
    if (int rc = launch_layernorm_backward(t.s2, ly.ln2_g, w->ln_eps, dy, dy_res, ws.d1, gr.ln2_g, gr.ln2_b, M, ws.partial, st)) return rc;
    if (int rc = launch_colsum(ws.d1, M, kD, gr.b_ffn2, ws.partial, st)) return rc;
    if (int rc = launch_gelu_forward(t.u, ws.act, M * ffn, st)) return rc;
    if (int rc = launch_gemm_tn(grad_weight(ws.d1, ws.act, gr.w_ffn2, M, kD, ffn), 1, st)) return rc;
    if (int rc = launch_gemm(grad_input(ws.d1, ly.w_ffn2, ws.big, M, kD, ffn), 1, true, st)) return rc;
    // GELU, FFN1
    if (int rc = launch_gelu_backward(ws.big, t.u, ws.big, M * ffn, st)) return rc;
    if (int rc = launch_colsum(ws.big, M, ffn, gr.b_ffn1, ws.partial, st)) return rc;
    if (int rc = launch_gemm_tn(grad_weight(ws.big, t.h, gr.w_ffn1, M, ffn, kD), 1, st)) return rc;
    if (int rc = launch_gemm(grad_input(ws.big, ly.w_ffn1, ws.d2, M, ffn, kD), 1, true, st)) return rc;
    // LN1 (dh = the FFN branch's gradient + ds2 down the residual), the output projection
    if (int rc = launch_layernorm_backward(t.s1, ly.ln1_g, w->ln_eps, ws.d2, ws.d1, ws.d3, gr.ln1_g, gr.ln1_b, M, ws.partial, st)) return rc;
    if (int rc = launch_colsum(ws.d3, M, kD, gr.b_o, ws.partial, st)) return rc;
    if (int rc = launch_gemm_tn(grad_weight(ws.d3, t.ctx, gr.w_o, M, kD, kD), 1, st)) return rc;
    if (int rc = launch_gemm(grad_input(ws.d3, ly.w_o, ws.d2, M, kD, kD), 1, true, st)) return rc;         // dctx
    // attention, per (document, head); dqkv = [dQ | dK | dV] in qkv's layout
    const long long s_qkv1 = (long long)L * 3 * kD, s_p1 = (long long)H * L * Lp, s_p2 = (long long)L * Lp, s_c1 = (long long)L * kD;
    GemmArgs g{};
    // dV_bh [keys, 64] = P_bh^T . dctx_bh
    g.A = t.probs; g.B = ws.d2; g.C = ws.dqkv + 2 * kD;
    g.M = (int)L; g.N = dh; g.K = (int)L; g.lda = Lp; g.ldb = kD; g.ldc = 3 * kD; g.nz2 = H; g.alpha = 1.f;
    g.sa1 = s_p1; g.sa2 = s_p2; g.sb1 = s_c1; g.sb2 = dh; g.sc1 = s_qkv1; g.sc2 = dh;
    if (int rc = launch_gemm_tn(g, batch, st)) return rc;
    // dP_bh [queries, keys] = dctx_bh . V_bh^T
    g = GemmArgs{};
    g.A = ws.d2; g.B = t.qkv + 2 * kD; g.C = ws.dprobs;
    g.M = (int)L; g.N = (int)L; g.K = dh; g.lda = kD; g.ldb = 3 * kD; g.ldc = Lp; g.nz2 = H; g.alpha = 1.f;
    g.sa1 = s_c1; g.sa2 = dh; g.sb1 = s_qkv1; g.sb2 = dh; g.sc1 = s_p1; g.sc2 = s_p2;
    if (int rc = launch_gemm(g, batch, false, st)) return rc;
    if (int rc = launch_softmax_backward(ws.dprobs, t.probs, B * H * L, (int)L, Lp, 1.0f / sqrtf((float)dh), st)) return rc;
    // dQ_bh = dS_bh . K_bh
    g = GemmArgs{};
    g.A = ws.dprobs; g.B = t.qkv + kD; g.C = ws.dqkv;
    g.M = (int)L; g.N = dh; g.K = (int)L; g.lda = Lp; g.ldb = 3 * kD; g.ldc = 3 * kD; g.nz2 = H; g.alpha = 1.f;
    g.sa1 = s_p1; g.sa2 = s_p2; g.sb1 = s_qkv1; g.sb2 = dh; g.sc1 = s_qkv1; g.sc2 = dh;
    if (int rc = launch_gemm(g, batch, true, st)) return rc;
    // dK_bh [keys, 64] = dS_bh^T . Q_bh
    g = GemmArgs{};
    g.A = ws.dprobs; g.B = t.qkv; g.C = ws.dqkv + kD;
    g.M = (int)L; g.N = dh; g.K = (int)L; g.lda = Lp; g.ldb = 3 * kD; g.ldc = 3 * kD; g.nz2 = H; g.alpha = 1.f;
    g.sa1 = s_p1; g.sa2 = s_p2; g.sb1 = s_qkv1; g.sb2 = dh; g.sc1 = s_qkv1; g.sc2 = dh;
    if (int rc = launch_gemm_tn(g, batch, st)) return rc;
    // the QKV projection
    if (int rc = launch_colsum(ws.dqkv, M, 3 * kD, gr.b_qkv, ws.partial, st)) return rc;
    if (int rc = launch_gemm_tn(grad_weight(ws.dqkv, t.x, gr.w_qkv, M, 3 * kD, kD), 1, st)) return rc;
    return launch_gemm(grad_input(ws.dqkv, ly.w_qkv, ws.d2, M, 3 * kD, kD), 1, true, st);
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

extern "C" int aspire_bert_layers_forward_train_f32(const aspire_bert_weights* w, const float* emb_sum, const int64_t* attn_mask, int64_t B,
                                                    int64_t L, float* hidden_out, void* tape, size_t tape_bytes, void* ws, size_t ws_bytes,
                                                    void* stream) {
    ASPIRE_REQUIRE(w && emb_sum && attn_mask && hidden_out, ASPIRE_ERR_INVALID_ARG, "null pointer");
    if (int rc = check_train_args(w, B, L)) return rc;
    if (B == 0) return ASPIRE_OK;
    const Geometry q = geometry(w, B, L);
    const size_t need_tape = carve_tape(nullptr, q).total, need_ws = carve_train(nullptr, q).total;
    ASPIRE_REQUIRE(tape && tape_bytes >= need_tape, ASPIRE_ERR_INVALID_ARG, "tape too small: need %zu bytes (aspire_bert_tape_bytes)", need_tape);
    ASPIRE_REQUIRE(ws && ws_bytes >= need_ws, ASPIRE_ERR_INVALID_ARG, "workspace too small: need %zu bytes (aspire_bert_train_workspace_bytes)",
                   need_ws);
    hipStream_t st = (hipStream_t)stream;
    const Tape t = carve_tape(tape, q);
    const TrainWorkspace tw = carve_train(ws, q);
    ASPIRE_HIP_OK(hipMemcpyAsync(t.emb(), emb_sum, (size_t)q.M * kD * sizeof(float), hipMemcpyDeviceToDevice, st));
    const int n = q.n_layers;
    if (int rc = launch_layernorm(t.emb(), w->emb_ln_g, w->emb_ln_b, w->ln_eps, n == 0 ? hidden_out : t.layer(0).x, q.M, nullptr, st)) return rc;
    for (int l = 0; l < n; ++l)
        if (int rc = forward_layer(w, q, l, t.layer(l), attn_mask, tw.act, l == n - 1 ? hidden_out : t.layer(l + 1).x, st)) return rc;
    return ASPIRE_OK;
}

extern "C" int aspire_bert_layers_backward_f32(const aspire_bert_weights* w, const int64_t* attn_mask, int64_t B, int64_t L,
                                               const float* grad_hidden, const void* tape, size_t tape_bytes, float* grad_emb_sum,
                                               const aspire_bert_grads* grads, void* ws, size_t ws_bytes, void* stream) {
    ASPIRE_REQUIRE(w && attn_mask && grad_hidden && grads, ASPIRE_ERR_INVALID_ARG, "null pointer");
    if (int rc = check_train_args(w, B, L)) return rc;
    ASPIRE_REQUIRE(grads->emb_ln_g && grads->emb_ln_b && (w->n_layers == 0 || grads->layers), ASPIRE_ERR_INVALID_ARG,
                   "null pointer in the gradient table");
    for (int l = 0; l < w->n_layers; ++l) {
        const aspire_bert_layer_grads& y = grads->layers[l];
        ASPIRE_REQUIRE(y.w_qkv && y.b_qkv && y.w_o && y.b_o && y.ln1_g && y.ln1_b && y.w_ffn1 && y.b_ffn1 && y.w_ffn2 && y.b_ffn2 && y.ln2_g &&
                           y.ln2_b,
                       ASPIRE_ERR_INVALID_ARG, "null pointer in layer %d's gradients", l);
    }
    if (B == 0) return ASPIRE_OK;
    const Geometry q = geometry(w, B, L);
    const size_t need_tape = carve_tape(nullptr, q).total, need_ws = carve_train(nullptr, q).total;
    ASPIRE_REQUIRE(tape && tape_bytes >= need_tape, ASPIRE_ERR_INVALID_ARG, "tape too small: need %zu bytes (aspire_bert_tape_bytes)", need_tape);
    ASPIRE_REQUIRE(ws && ws_bytes >= need_ws, ASPIRE_ERR_INVALID_ARG, "workspace too small: need %zu bytes (aspire_bert_train_workspace_bytes)",
                   need_ws);
    hipStream_t st = (hipStream_t)stream;
    const Tape t = carve_tape(tape, q);
    const TrainWorkspace tw = carve_train(ws, q);
    const float *dy = grad_hidden, *dy_res = nullptr;
    for (int l = q.n_layers - 1; l >= 0; --l) {
        if (int rc = backward_layer(w, q, l, t.layer(l), grads->layers[l], dy, dy_res, tw, st)) return rc;
        dy = tw.d2;         // the attention branch's gradient of the layer's input ...
        dy_res = tw.d3;     // ... and ds1 down the residual: summed by the LayerNorm backward that reads them
    }
    // the embedding LayerNorm (grad_emb_sum NULL: its input gradient goes to scratch, the parameter gradients are still wanted)
    return launch_layernorm_backward(t.emb(), w->emb_ln_g, w->ln_eps, dy, dy_res, grad_emb_sum ? grad_emb_sum : tw.d1, grads->emb_ln_g,
                                     grads->emb_ln_b, q.M, tw.partial, st);
}
