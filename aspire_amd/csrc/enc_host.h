// Host side that the encoder's two host files share (encoder.hip: inference and the CLS forward; encoder_bwd.hip: the layer stack under
// training): the buffer carver, the GemmArgs builders, the three-kernel attention, the fp32-operand layer tail and the argument checks
// both make.  Every fp32-operand launch sequence of a BERT layer is written here once.  Host only: no kernel, nothing a kernel reads
// beyond the GemmArgs the builders return; plain C++ over the launchers enc_types.h declares.
#pragma once
#include <math.h>

#include "enc_types.h"

namespace aspire {

// The three operand forms of a product C [M, N] = A . B over K (GemmArgs): NT A [M, K] and B [N, K], both k-contiguous (launch_gemm);
// B_KN B [K, N] n-contiguous (launch_gemm's b_kn); TN A [K, M] and B [K, N] (launch_gemm_tn).  The values are the C ABI's
// (aspire_debug_gemm_bf16_f32's `form`).
enum { kGemmNT = 0, kGemmBKN = 1, kGemmTN = 2 };

// enc_gemm_bf16.hip: the same product with every operand element rounded to bf16 once, when its tile is staged, on the bf16 matrix
// cores with fp32 accumulators and the fp32 epilogues of launch_gemm; any M, N, K, lda / ldb multiples of 4 (ASPIRE_MATMUL_BF16)
int launch_gemm_bf16(const GemmArgs& g, int batch, int form, hipStream_t st);

// enc_gemm_bf16x3.hip: the B_KN and TN forms at fp32 accuracy on the bf16 matrix cores -- every operand element split into three bf16
// planes when its tile is staged, six products per term, fp32 accumulators (the TN form in two levels) and the same epilogues; any
// M, N, K, lda / ldb multiples of 4.  The NT form goes to launch_gemm, which is that arithmetic already wherever K % 16 == 0
// (ASPIRE_MATMUL_BF16X3)
int launch_gemm_bf16x3(const GemmArgs& g, int batch, int form, hipStream_t st);

namespace {

// A product of the layer stack in the caller's matmul mode: ASPIRE_MATMUL_FP32 launches what the stack always launched
int launch_product(int matmul, const GemmArgs& g, int batch, int form, hipStream_t st) {
    if (matmul == ASPIRE_MATMUL_BF16) return launch_gemm_bf16(g, batch, form, st);
    if (matmul == ASPIRE_MATMUL_BF16X3) return launch_gemm_bf16x3(g, batch, form, st);
    return form == kGemmTN ? launch_gemm_tn(g, batch, st) : launch_gemm(g, batch, form == kGemmBKN, st);
}

// The argument checks of the aspire_debug_gemm_*_f32 entries (include/aspire_hip.h) and the GemmArgs they launch.  *launch = false: a
// zero size, nothing to do.
int debug_gemm_args(const float* A, const float* B, float* C, int64_t M, int64_t N, int64_t K, int64_t lda, int64_t ldb, int64_t ldc, int form,
                    int64_t batch, int64_t nz2, int64_t sa1, int64_t sa2, int64_t sb1, int64_t sb2, int64_t sc1, int64_t sc2, float alpha,
                    const float* bias, const float* res, int64_t ldr, int gelu, GemmArgs* out, bool* launch) {
    *launch = false;
    ASPIRE_REQUIRE(A && B && C, ASPIRE_ERR_INVALID_ARG, "null pointer (A / B / C)");
    ASPIRE_REQUIRE(M >= 0 && N >= 0 && K >= 0 && batch >= 0, ASPIRE_ERR_INVALID_ARG, "negative size (M %lld N %lld K %lld batch %lld)",
                   (long long)M, (long long)N, (long long)K, (long long)batch);
    ASPIRE_REQUIRE(form == kGemmNT || form == kGemmBKN || form == kGemmTN, ASPIRE_ERR_INVALID_ARG, "unknown GEMM form %d (0 NT, 1 B_KN, 2 TN)",
                   form);
    ASPIRE_REQUIRE(nz2 >= 1, ASPIRE_ERR_INVALID_ARG, "nz2 = %lld: the inner batch count is at least 1", (long long)nz2);
    // what each operand's rows must span, and the float4 rule of the fp32 forms
    const int64_t a_cols = form == kGemmTN ? M : K, b_cols = form == kGemmNT ? K : N;
    ASPIRE_REQUIRE(lda >= a_cols && ldb >= b_cols && ldc >= N && (!res || ldr >= N), ASPIRE_ERR_INVALID_ARG,
                   "a leading dimension is shorter than its row (lda %lld ldb %lld ldc %lld ldr %lld)", (long long)lda, (long long)ldb,
                   (long long)ldc, (long long)ldr);
    ASPIRE_REQUIRE(lda % 4 == 0 && ldb % 4 == 0 && (sa1 | sa2 | sb1 | sb2) % 4 == 0 && (((uintptr_t)A | (uintptr_t)B) & 15) == 0,
                   ASPIRE_ERR_INVALID_ARG, "A and B are read as float4: 16-byte aligned bases, lda / ldb / batch strides multiples of 4");
    ASPIRE_REQUIRE(M < (1 << 30) && N < (1 << 30) && K < (1 << 30) && lda < (1 << 30) && ldb < (1 << 30) && ldc < (1 << 30) && ldr < (1 << 30) &&
                       batch <= 65535,
                   ASPIRE_ERR_UNSUPPORTED, "a size beyond the kernel's 32-bit indices (or more than 65535 matrices)");
    if (M == 0 || N == 0 || K == 0 || batch == 0) return ASPIRE_OK;
    GemmArgs g{};
    g.A = A; g.B = B; g.C = C; g.bias = bias; g.res = res;
    g.M = (int)M; g.N = (int)N; g.K = (int)K; g.lda = (int)lda; g.ldb = (int)ldb; g.ldc = (int)ldc; g.ldr = (int)ldr;
    g.nz2 = (int)nz2; g.sa1 = sa1; g.sa2 = sa2; g.sb1 = sb1; g.sb2 = sb2; g.sc1 = sc1; g.sc2 = sc2;
    g.alpha = alpha; g.gelu = gelu ? 1 : 0;
    *out = g;
    *launch = true;
    return ASPIRE_OK;
}

size_t align_up(size_t x) { return (x + 255) & ~(size_t)255; }

// Carves 256-byte-aligned slots off a buffer, in call order.  A null base only measures: every slot is null and `off` ends at the
// bytes a real buffer needs.
struct Carver {
    char* base;
    size_t off = 0;
    explicit Carver(const void* b) : base((char*)b) {}
    void* bytes(size_t n) {
        void* r = base ? base + off : nullptr;
        off += align_up(n);
        return r;
    }
    float* floats(size_t n) { return (float*)bytes(n * sizeof(float)); }
};

// C [rows, N] = A [rows, K] . W [N, K]^T (+ bias) (+ GELU) (+ res [rows, N]): the nn.Linear form
GemmArgs linear(const float* A, const float* W, float* C, const float* bias, const float* res, int64_t rows, int N, int K, bool gelu = false) {
    GemmArgs g{};
    g.A = A; g.B = W; g.C = C; g.bias = bias; g.res = res; g.ldr = N;
    g.M = (int)rows; g.N = N; g.K = K; g.lda = K; g.ldb = K; g.ldc = N; g.nz2 = 1; g.alpha = 1.f;
    g.gelu = gelu ? 1 : 0;
    return g;
}

// One matrix per (document, head) inside a buffer that holds all of them: row stride, document stride, head stride (floats)
template <class T>
struct Heads {
    T* p;
    int ld;
    long long s1, s2;
};
// Q, K or V (p = qkv, qkv + 768, qkv + 1536) of the fused projection [B L, 2304], and their gradients in the same layout
template <class T>
Heads<T> qkv_heads(T* p, int64_t L, int dh) { return {p, 3 * kD, (long long)L * 3 * kD, dh}; }
// scores / probabilities [B, H, L, Lp]
template <class T>
Heads<T> prob_heads(T* p, int H, int64_t L, int Lp) { return {p, Lp, (long long)H * L * Lp, (long long)L * Lp}; }
// the attention context [B L, 768], head h in columns [h dh, (h + 1) dh)
template <class T>
Heads<T> ctx_heads(T* p, int64_t L, int dh) { return {p, kD, (long long)L * kD, dh}; }

// the batched product C_bh [M, N] = A_bh . B_bh over K, one per (document, head): launch with batch = B H.  Which of the three forms
// it is (B as [N, K], as [K, N], or A transposed) is the launcher's to say (launch_gemm's b_kn, launch_gemm_tn).
template <class TA, class TB>
GemmArgs head_gemm(Heads<TA> A, Heads<TB> B, Heads<float> C, int64_t M, int64_t N, int64_t K, int H) {
    GemmArgs g{};
    g.A = A.p; g.B = B.p; g.C = C.p;
    g.M = (int)M; g.N = (int)N; g.K = (int)K; g.lda = A.ld; g.ldb = B.ld; g.ldc = C.ld; g.nz2 = H; g.alpha = 1.f;
    g.sa1 = A.s1; g.sa2 = A.s2; g.sb1 = B.s1; g.sb2 = B.s2; g.sc1 = C.s1; g.sc2 = C.s2;
    return g;
}

// Steps 2 - 4 of a layer in the three-kernel form: qkv [B L, 2304] -> probs [B, H, L, Lp] (the soft-max probabilities stay there, pad
// columns zero) -> ctx [B L, 768].  With `drop` (training, p_attn > 0): the probabilities stay undropped in `probs` (the soft-max
// backward wants them), their dropped copy goes to `dropped` (same layout) and the P.V product reads that.
int attention_gemm(const float* qkv, float* probs, float* ctx, const int64_t* mask, int64_t B, int64_t L, int Lp, int H, int dh,
                   const float* rel_bias, int rel_span, hipStream_t st, const DropSite* drop = nullptr, float* dropped = nullptr,
                   int matmul = ASPIRE_MATMUL_FP32) {
    const int batch = (int)(B * H);
    // 2. scores[b,h] = Q_bh . K_bh^T   (scale and mask are applied by the softmax kernel)
    if (int rc = launch_product(matmul, head_gemm(qkv_heads(qkv, L, dh), qkv_heads(qkv + kD, L, dh), prob_heads(probs, H, L, Lp), L, L, dh, H), batch,
                                kGemmNT, st))
        return rc;
    // 3. masked softmax over keys, in place
    if (int rc = launch_softmax_mask(probs, mask, B * H * L, (int)L, Lp, (int)(H * L), 1.0f / sqrtf((float)dh), rel_bias, rel_span, st)) return rc;
    if (drop) {
        if (int rc = launch_dropout_probs(probs, dropped, B * H * L, (int)L, Lp, *drop, st)) return rc;
        probs = dropped;
    }
    // 4. ctx[b, :, h*64:(h+1)*64] = P_bh . V_bh        (V is [K = L keys, N = 64] n-contiguous)
    return launch_product(matmul, head_gemm(prob_heads(probs, H, L, Lp), qkv_heads(qkv + 2 * kD, L, dh), ctx_heads(ctx, L, dh), L, dh, L, H), batch,
                          kGemmBKN, st);
}

// Where the layer tail leaves its intermediates, [rows, 768] each but u and act [rows, ffn_dim]
struct TailSlots {
    float* s1;      // ctx . Wo^T + bo + x, the pre-LN1 sum
    float* h;       // LN1(s1)
    float* u;       // h . W1^T + b1 before the GELU, or NULL when nobody reads it
    float* act;     // GELU(u)
    float* s2;      // act . W2^T + b2 + h, the pre-LN2 sum
};

// Steps 5 - 6 of a layer on fp32 operands, behind any attention form: ctx (the attention context) and x (the layer's input) [rows, 768]
// -> out = LN2(GELU(h W1^T + b1) W2^T + b2 + h), h = LN1(ctx Wo^T + bo + x).  With t.u the FFN1 GEMM runs with its GELU epilogue off and
// the activation is a pass of its own (the same gelu_erf on the same fp32 value: the same bits), so that the pre-GELU value is kept
// (training); without, the epilogue writes act directly (inference).  Slots may share a buffer wherever the earlier one is dead by the
// time the later one is written -- the launches are stream-ordered and none reads what it writes: s2 may be s1, out may be x, and h may
// be ctx (the out-projection that reads ctx has finished before LN1 writes h: inference runs so).
// `matmul` (ASPIRE_MATMUL_*, here and in attention_gemm): the mode of the products alone; every other launch is the same.
// With `drop` (training, p_hidden > 0; drop[0]: the out-projection's site, drop[1]: FFN2's) the two GEMMs run with their bias and
// WITHOUT the residual, and a pass of its own forms s = dropout(z) + residual in the same slot.  row_map (the padding-free mode, whose
// rows are the valid tokens alone): the padded row of each row, which keys its masks.
int layer_tail(const aspire_bert_weights* w, const aspire_bert_layer& ly, const float* ctx, const float* x, const TailSlots& t, float* out,
               int64_t rows, hipStream_t st, const DropSite* drop = nullptr, int matmul = ASPIRE_MATMUL_FP32, const int32_t* row_map = nullptr) {
    const int ffn = w->ffn_dim;
    // 5. attention output projection + residual, LayerNorm
    if (int rc = launch_product(matmul, linear(ctx, ly.w_o, t.s1, ly.b_o, drop ? nullptr : x, rows, kD, kD), 1, kGemmNT, st)) return rc;
    if (drop)
        if (int rc = launch_dropout_flat(t.s1, nullptr, x, t.s1, rows * kD, drop[0], st, row_map)) return rc;
    if (int rc = launch_layernorm(t.s1, ly.ln1_g, ly.ln1_b, w->ln_eps, t.h, rows, nullptr, st)) return rc;
    // 6. FFN: GELU(h . W1^T + b1) . W2^T + b2 + h, LayerNorm
    if (t.u) {
        if (int rc = launch_product(matmul, linear(t.h, ly.w_ffn1, t.u, ly.b_ffn1, nullptr, rows, ffn, kD), 1, kGemmNT, st)) return rc;
        if (int rc = launch_gelu_forward(t.u, t.act, rows * ffn, st)) return rc;
    } else {
        if (int rc = launch_product(matmul, linear(t.h, ly.w_ffn1, t.act, ly.b_ffn1, nullptr, rows, ffn, kD, true), 1, kGemmNT, st)) return rc;
    }
    if (int rc = launch_product(matmul, linear(t.act, ly.w_ffn2, t.s2, ly.b_ffn2, drop ? nullptr : t.h, rows, kD, ffn), 1, kGemmNT, st)) return rc;
    if (drop)
        if (int rc = launch_dropout_flat(t.s2, nullptr, t.h, t.s2, rows * kD, drop[1], st, row_map)) return rc;
    return launch_layernorm(t.s2, ly.ln2_g, ly.ln2_b, w->ln_eps, out, rows, nullptr, st);
}

// What every forward and the backward check of the weights' geometry and the shape, before anything else of w is read
int check_bert_shape(const aspire_bert_weights* w, int64_t B, int64_t L) {
    ASPIRE_REQUIRE(w->hidden == kD && w->n_heads == 12 && w->ffn_dim % 64 == 0 && w->ffn_dim > 0, ASPIRE_ERR_UNSUPPORTED,
                   "only BERT-base geometry is built (hidden 768, 12 heads, ffn_dim %% 64 == 0); got hidden %d heads %d ffn_dim %d", w->hidden,
                   w->n_heads, w->ffn_dim);
    ASPIRE_REQUIRE(B >= 0 && L > 0 && L <= 512, ASPIRE_ERR_INVALID_ARG, "sequence length %lld outside (0, 512] (or a negative batch size)",
                   (long long)L);
    ASPIRE_REQUIRE(w->n_layers >= 0 && (w->n_layers == 0 || w->layers), ASPIRE_ERR_INVALID_ARG, "bad layer table");
    return ASPIRE_OK;
}

// The caller's packing (include/aspire_hip.h: aspire_bert_packing) of a [B, L] batch, checked on the host before anything is read
// through it, as what the kernels take.  The lists themselves are device memory: the kernels clamp what they read from them.
int read_packing(const aspire_bert_packing* p, int64_t B, int64_t L, PackedDocs* out) {
    ASPIRE_REQUIRE(p, ASPIRE_ERR_INVALID_ARG, "null pointer (packing)");
    ASPIRE_REQUIRE(p->doc_start && (p->row_src || p->rows == 0) && (p->row_dst || B == 0), ASPIRE_ERR_INVALID_ARG,
                   "null pointer (packing: doc_start / row_src / row_dst)");
    ASPIRE_REQUIRE(B >= 0 && L > 0 && (double)B * (double)L < 2147483648.0, ASPIRE_ERR_UNSUPPORTED,
                   "%lld x %lld padded token rows: the row lists are 32-bit (split the batch)", (long long)B, (long long)L);
    ASPIRE_REQUIRE(p->rows >= 0 && p->rows <= B * L, ASPIRE_ERR_INVALID_ARG, "packing: %lld rows of a batch of %lld x %lld", (long long)p->rows,
                   (long long)B, (long long)L);
    ASPIRE_REQUIRE(p->max_len >= 0 && p->max_len <= L && p->max_len <= p->rows && (p->max_len > 0) == (p->rows > 0), ASPIRE_ERR_INVALID_ARG,
                   "packing: longest document %d with %lld rows of %lld-token documents", (int)p->max_len, (long long)p->rows, (long long)L);
    *out = PackedDocs{p->doc_start, p->row_src, (int)p->rows, (int)L, (p->prefix != 0 && L % 4 == 0) ? 1 : 0};
    return ASPIRE_OK;
}

// No null among the twelve pointers of each of n aspire_bert_layer / aspire_bert_layer_grads (the two structs name the same fields)
template <class Layer>
int check_layer_pointers(const Layer* layers, int n, const char* what) {
    for (int l = 0; l < n; ++l) {
        const Layer& y = layers[l];
        ASPIRE_REQUIRE(y.w_qkv && y.b_qkv && y.w_o && y.b_o && y.ln1_g && y.ln1_b && y.w_ffn1 && y.b_ffn1 && y.w_ffn2 && y.b_ffn2 && y.ln2_g &&
                           y.ln2_b,
                       ASPIRE_ERR_INVALID_ARG, "null pointer in layer %d's %s", l, what);
    }
    return ASPIRE_OK;
}

}  // namespace
}  // namespace aspire
