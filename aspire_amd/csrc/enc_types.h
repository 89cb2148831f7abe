// What the encoder's units share: the argument structs the GEMM kernels take by value (GemmArgs: filled by enc_host.h's builders and
// encoder_bwd.hip's two gradient forms; PGemmArgs: by run_layer in encoder.hip), the two device-side names that kernels of more than
// one unit use, and the host launchers each kernel family's unit offers to the two host files, encoder.hip and encoder_bwd.hip (one
// comment line names the unit).  What those two share on the host side is enc_host.h; the fp16-plane layout has a header of its own,
// enc_planes.h.
#pragma once
#include "common.h"
#include "dropout_rng.h"

namespace aspire {

struct GemmArgs {
    const float* A;     // [batch][M][lda]
    const float* B;     // B_KN ? [batch][K][ldb] : [batch][N][ldb]
    float* C;           // [batch][M][ldc]
    const float* bias;  // [N] or null
    const float* res;   // [M][ldr] residual or null (not batched)
    int M, N, K;
    int lda, ldb, ldc, ldr;
    // batch index z = z1 * nz2 + z2; operand offsets are z1 * s?1 + z2 * s?2 (attention: z1 = doc, z2 = head)
    int nz2;
    long long sa1, sa2, sb1, sb2, sc1, sc2;
    float alpha;
    int gelu;
};

struct PGemmArgs {
    const void* Ap;      // P layout [M, K]
    const void* Bp;      // P layout [N, K] (nn.Linear weight, scaled by kPWeightScale)
    float* C;            // fp32 [M, ldc] out (F32 epilogue)
    void* Cp;            // P layout [M, N] out (GELU_P epilogue: the next GEMM's A operand, its k dimension = N)
    const float* bias;   // [N] or null
    const float* res;    // [M, ldr] residual or null
    int M, N, K, ldc, ldr;
    int n_off;           // first column of this launch (a GEMM may run as a launch of 128-wide and one of 64-wide column tiles)
    int probe;           // timing probes (ASPIRE_HIP_GEMM_PROBE): 1 no MFMAs, 2 no LDS-DMA
    int tiles_x, tiles_y;   // PERSIST / LN: the tile grid (PERSIST: a workgroup walks several tiles; the launch grid is the resident workgroups)
    // LN epilogue (N = 768 = the whole row): y = LayerNorm(acc + bias + residual) * gamma + beta -> C (fp32, optional) and Cp (P layout,
    // optional); the residual is READ from a P layout [M, 768] (resp; h + l = the fp32 value to fp32's own rounding) and may BE Cp:
    // every 8-byte slot is read and later written by the one lane that owns it
    const void* resp;
    const float *gamma, *beta;
    float eps;
    float2* ln_stats;    // [M][768 / BN] (mean, sum of squared deviations) of a row's BN columns, one entry per column tile
    int* ln_count;       // [row blocks] zeroed before the launch: column tiles of the row block that have published their entry
    // QKV epilogue (EPI 1, launch_gemm_p_qkv): the attention kernel's operands, already split -- Xp = the planes
    // [plane h | l][Q | K | V][head][M][64] fp16 (flash_attn_p_kernel)
    void* Xp;
};

// The fp16 matmul mode's GEMM (enc_gemm_h.hip) on single-plane fp16 operands (the H layout: enc_hplane.h)
struct HGemmArgs {
    const void* Ah;      // H layout [M, K]
    const void* Bh;      // H layout [N, K] (nn.Linear weight, scaled by kPWeightScale)
    float* C;            // fp32 [M, ldc] out (epilogue a)
    void* Ch;            // H layout [M, N] out (epilogue b: GELU(.), the next GEMM's A operand, its k dimension = N)
    const float* bias;   // [N] or null
    const float* res;    // [M, ldr] fp32 residual or null (epilogue a)
    int M, N, K, ldc, ldr;
    int n_off;           // first column of this launch (set by the launcher: a GEMM may run as 128-wide and 64-wide column tiles)
};

namespace {

using f32x16 = __attribute__((ext_vector_type(16))) float;

// GELU as HF BertModel's "gelu" (0.5 x (1 + erf(x / sqrt 2))), written around erfc: e = erfc(|x| / sqrt 2) = 2^q(|x|), q a degree-8 polynomial
// (a weighted Chebyshev fit of log2 erfc(t / sqrt 2) on [0, 5.8]; beyond, erfc < 7e-9), then x - 0.5 x e for x > 0 and 0.5 x e otherwise: no
// cancellation on either side, 15 VALU instructions where 0.5 x (1 + erff(.)) takes 37 (50 M activations per FFN1 launch at 64 x 256 tokens).
// Max |error| against float64 over [-9, 9]: 2.5e-7 (the erff form, rounded in fp32: 4.5e-7).
__device__ __forceinline__ float gelu_erf(float x) {
    const float t = fminf(fabsf(x), 5.8f);
    float q = -1.9605818124546204e-06f;
    q = fmaf(q, t, 2.8825294066336937e-05f);
    q = fmaf(q, t, -0.0001355033746222034f);
    q = fmaf(q, t, -0.0002612900862004608f);
    q = fmaf(q, t, 0.007229907438158989f);
    q = fmaf(q, t, -0.05261624604463577f);
    q = fmaf(q, t, -0.4591653645038605f);
    q = fmaf(q, t, -1.1511112451553345f);
    q = fmaf(q, t, 1.7379414884999278e-07f);
    const float r = 0.5f * x * __builtin_amdgcn_exp2f(q);
    return x > 0.f ? x - r : r;
}

}  // namespace

// enc_gemm.hip: C = alpha A.B^T (+bias)(+GELU)(+residual) on fp32 operands, batched; b_kn: B is [K, N] n-contiguous (V of attention)
int launch_gemm(const GemmArgs& g, int batch, bool b_kn, hipStream_t st);
// the TN form on the fp32-input matrix cores: C[M, N] = alpha sum_r A[r, M] . B[r, N] (+ the same epilogues); g.A is [batch][K][lda],
// g.B [batch][K][ldb], both row-major with the contraction over their rows; M, N, lda, ldb multiples of 4 (encoder_bwd.hip)
int launch_gemm_tn(const GemmArgs& g, int batch, hipStream_t st);

// enc_gemm_p.hip: the GEMMs on pre-split fp16 planes (enc_planes.h) and the split of an fp32 matrix into them (weight: the B side,
// scaled by kPWeightScale; too_big: optional device flag).  swap: the GELU -> P-layout epilogue.  The unit also owns the encoder's
// device globals and the entry points that touch them: aspire_bert_status, aspire_debug_gemm_buffer.
int launch_split_planes(const float* X, int64_t R, int K, void* P, bool weight, int* too_big, hipStream_t st);
int launch_gemm_p(const PGemmArgs& g, bool swap, hipStream_t st);
int launch_gemm_p_qkv(PGemmArgs g, hipStream_t st);
int launch_gemm_p_ln(const PGemmArgs& g, hipStream_t st);
bool ln_fused_supported();

// enc_gemm_h.hip: the fp16 matmul mode of the inference encoder (ASPIRE_MATMUL_FP16) -- the GEMM on single-plane fp16 operands (gelu_h:
// epilogue b, GELU -> g.Ch; else epilogue a -> g.C; any M >= 1, N % 64 == 0, K % 32 == 0), an fp32 matrix (row stride ld) into the H
// layout (weight: the B side, scaled by kPWeightScale; too_big: optional device flag), and the LayerNorm that writes the fp32 row and
// its H copy (yh, optional) in one pass.  No device globals, no atomics.
int launch_gemm_h(const HGemmArgs& g, bool gelu_h, hipStream_t st);
int launch_split_h(const float* X, int64_t R, int K, int64_t ld, void* H, bool weight, int* too_big, hipStream_t st);
int launch_layernorm_h(const float* x, const float* gamma, const float* beta, float eps, float* y, int64_t rows, void* yh, hipStream_t st);

// enc_attn.hip: the masked soft-max of the three-kernel form, fused attention on fp32 Q / K / V (f32: fp32-input MFMAs, else fp16
// planes split in the kernel) and on the QKV GEMM's planes (keys64: 64-key tiles), and the CLS query's attention.
// rel_bias [H][2 rel_span - 1] or NULL: aspire_bert_extras' relative-position bias (keys64 with it: ASPIRE_ERR_UNSUPPORTED)
int launch_softmax_mask(float* s, const int64_t* mask, int64_t rows, int L, int ld, int rows_per_doc, float scale, const float* rel_bias,
                        int rel_span, hipStream_t st);
int launch_flash_attn(const float* qkv, const int64_t* mask, float* ctx, int64_t B, int L, int H, void* ctxp, int64_t rows, bool f32,
                      const float* rel_bias, int rel_span, hipStream_t st);
int launch_flash_attn_p(const unsigned char* qkvp, const int64_t* mask, float* ctx, int64_t B, int L, int H, void* ctxp, int64_t rows,
                        bool keys64, const float* rel_bias, int rel_span, hipStream_t st);
int launch_cls_attn(const float* qkv, const unsigned char* qkvp, const int64_t* mask, float* ctx, int64_t B, int L, int H, int64_t rows,
                    hipStream_t st);

// enc_attn_train.hip: the fused attention of the training encoder (ASPIRE_ATTENTION_FLASH; bf16 operands, fp32 everywhere else).
// Forward: qkv [B L, 2304] -> ctx [B L, 768] and stats [B, H, L, 2] = per query the row maximum (log2 units) and the undropped row sum.
// Backward: D [B, H, L] (scratch) = rowsum(dctx . ctx), then dqkv [B L, 2304] = [dQ | dK | dV], every element written once.
// drop: the layer's attention site or NULL (no generator in the kernels).  H = 12, L in 1 .. 512.
int launch_flash_attn_train(const float* qkv, const int64_t* mask, float* ctx, float* stats, int64_t B, int L, int H, const DropSite* drop,
                            hipStream_t st);
int launch_flash_attn_train_backward(const float* qkv, const int64_t* mask, const float* ctx, const float* stats, const float* dctx, float* D,
                                     float* dqkv, int64_t B, int L, int H, const DropSite* drop, hipStream_t st);
// The same kernels over PACKED rows (ASPIRE padding-free mode): the row tensors hold the `rows` valid tokens alone, document b's at
// rows doc_start[b] .. doc_start[b + 1] - 1 in position order; qkv / dqkv [rows, 2304], ctx / dctx [rows, 768], stats [H, rows, 2],
// D [H, rows].  row_src[m] = b Lpad + (the token's position in its padded document): what the dropout keys are made of, so that the
// masks are the padded call's.  quad: every document is a prefix and Lpad % 4 == 0 (one draw per four keys where the lane is a query).
// No mask is read: every key of a document is real.  max_len: the longest document (the grid's blocks); 0 launches nothing.
struct PackedDocs {
    const int32_t* doc_start;   // [B + 1]
    const int32_t* row_src;     // [rows]
    int rows, Lpad, quad;
};
int launch_flash_attn_train_packed(const float* qkv, const PackedDocs& docs, int max_len, float* ctx, float* stats, int64_t B, int H,
                                   const DropSite* drop, hipStream_t st);
int launch_flash_attn_train_backward_packed(const float* qkv, const PackedDocs& docs, int max_len, const float* ctx, const float* stats,
                                            const float* dctx, float* D, float* dqkv, int64_t B, int H, const DropSite* drop, hipStream_t st);

// enc_pack.hip: the gather and scatter between the padded [B L, 768] layout and the packed [rows, 768] one (one wave per row, 16-byte
// accesses, every output row written once)
//   pack_rows:    out[m, :] = src[row_src[m], :], m < rows
//   unpack_rows:  out[p, :] = row_dst[p] >= 0 ? src[row_dst[p], :] : 0, p < padded_rows (no zero fill in front)
int launch_pack_rows(const float* src, const int32_t* row_src, float* out, int64_t rows, int64_t padded_rows, hipStream_t st);
int launch_unpack_rows(const float* src, const int32_t* row_dst, float* out, int64_t padded_rows, int64_t rows, hipStream_t st);

// enc_rows.hip: one wave per row of 768 -- LayerNorm, embeddings + LayerNorm (pos_ids [rows] or NULL: the row of pos each token takes,
// NULL = its index in the document), the CLS rows of a hidden state
int launch_layernorm(const float* x, const float* gamma, const float* beta, float eps, float* y, int64_t rows, void* yp, hipStream_t st);
int launch_embed_layernorm(const int64_t* tok, const int64_t* typ, const int64_t* pos_ids, const float* word, const float* pos,
                           const float* type_emb, const float* gamma, const float* beta, float eps, float* y, int64_t rows, int64_t L,
                           void* yp, hipStream_t st);
int launch_cls_tap(const float* x, const void* xp, int64_t rows, int64_t L, int64_t B, float wt, int mode, float* cls_out, float* layer_cls,
                   float* gather, hipStream_t st);

// enc_bwd.hip: the row kernels of the encoder's backward (encoder_bwd.hip runs them).  No atomics: every output element has one writer,
// column sums go through per-row-block partials (`partial`) and a fixed-order second stage.
//   gelu_forward:        a = GELU(u), n elements (the training forward's own GELU pass: the pre-GELU value stays on the tape)
//   gelu_backward:       du = dy . GELU'(u), n elements; du may be dy
//   softmax_backward:    ds[row][j] = scale . p[row][j] (dp[row][j] - sum_j dp p), j < L; zeros in [L, ld); in place (ds = dp)
//   layernorm_backward:  x the saved pre-norm rows; dy (+ dy_res when not NULL) the gradient of the LayerNorm's output; dx out;
//                        dgamma / dbeta [768] out through partial (layernorm_backward_partial_floats(rows))
//   colsum:              out[n] = sum_m x[m][n], x [rows, N] contiguous, through partial (colsum_partial_floats(rows, N))
int launch_gelu_forward(const float* u, float* a, int64_t n, hipStream_t st);
int launch_gelu_backward(const float* dy, const float* u, float* du, int64_t n, hipStream_t st);
int launch_softmax_backward(float* dp, const float* p, int64_t rows, int L, int ld, float scale, hipStream_t st);
size_t layernorm_backward_partial_floats(int64_t rows);
int launch_layernorm_backward(const float* x, const float* gamma, float eps, const float* dy, const float* dy_res, float* dx, float* dgamma,
                              float* dbeta, int64_t rows, float* partial, hipStream_t st);
size_t colsum_partial_floats(int64_t rows, int N);
int launch_colsum(const float* x, int64_t rows, int N, float* out, float* partial, hipStream_t st);

// enc_dropout.hip: the dropout passes of the encoder under training; d names the site and its mask (dropout_rng.h), which every pass
// forms again from the element's logical index.  No atomics, every output element has one writer; out may be the first operand.
//   dropout_flat:   out = keep . scale . (a (+ a2)) (+ res), n % 4 == 0 contiguous elements whose logical index is their offset; with
//                   row_map (packed rows of 768: n = rows x 768) element (m, c) is keyed as row_map[m] x 768 + c instead
//   dropout_probs:  out [rows][ld] = keep . scale . p [rows][ld] with logical index row L + j, j < L; zeros in [L, ld)
//   dropout_mask:   keep[i] = 1 iff element first + i of the site is kept
int launch_dropout_flat(const float* a, const float* a2, const float* res, float* out, int64_t n, const DropSite& d, hipStream_t st,
                        const int32_t* row_map = nullptr);
int launch_dropout_probs(const float* p, float* out, int64_t rows, int L, int ld, const DropSite& d, hipStream_t st);
int launch_dropout_mask(unsigned char* keep, uint64_t first, int64_t n, const DropSite& d, hipStream_t st);

// enc_cls_train.hip: the CLS read-out of a training forward, its gradient source, and the in-batch cross-entropy of two towers' CLS
// rows.  No atomics, every output element has one writer.
//   ClsStates:       where the n_layers + 1 hidden states of a training forward lie: state l < n_layers at x0 + l * layer_stride bytes
//                    (the tape's layer inputs), state n_layers at top (hidden_out); [B, L, 768] each
//   cls_mix_tap:     layer_cls [n_layers + 1, B, 768] (when not NULL) = the states' CLS rows; cls_out [B, 768] = sum_l mix[l] . row_l,
//                    l ascending (mix NULL: the top state's rows, copied)
//   cls_inject:      grad[b, 0, :] += (mix ? mix[l] : 1) . grad_cls[b, :] on a [B, L, 768] gradient
//   cls_grad_mix:    grad_mix[l] = sum_b <grad_cls[b], layer_cls[l, b]>, l < n_states (summed in double, rounded once)
//   inbatch_xent:    row_lse[i] = logsumexp_j <q_i, c_j>, loss[0] = sum_i (row_lse[i] - <q_i, c_i>); B <= kXentMaxRows rows of 768
//   inbatch_xent_backward: grad_q[i] = sum_j W_ij c_j, grad_c[j] = sum_i W_ij q_i, W_ij = grad_loss[0] (softmax_j(s_i.)_j - [i == j]),
//                    the soft-max formed again from the same products (nothing is read from the forward)
constexpr int kXentMaxRows = 128;
struct ClsStates {
    const char* x0;
    size_t layer_stride;
    const float* top;
    int n_layers;
};
//   ClsRows:         packed states (the padding-free mode): document b's CLS row is its first packed row doc_start[b] of the [rows, 768]
//                    states on the tape; the top state stays padded ([B, L, 768], hidden_out), where that row is row_src[doc_start[b]].
//                    NULL: the padded layout, row b L everywhere
struct ClsRows {
    const int32_t* doc_start;
    const int32_t* row_src;
    int rows, padded_rows;      // rows > 0; padded_rows = B L
};
int launch_cls_mix_tap(const ClsStates& s, int64_t B, int64_t L, const float* mix, float* cls_out, float* layer_cls, hipStream_t st,
                       const ClsRows* packed = nullptr);
int launch_cls_inject(float* grad, int64_t B, int64_t L, const float* grad_cls, const float* mix, int l, hipStream_t st,
                      const ClsRows* packed = nullptr);
int launch_cls_grad_mix(const float* grad_cls, const float* layer_cls, int64_t B, int n_states, float* grad_mix, hipStream_t st);
int launch_inbatch_xent(const float* q, const float* c, int B, float* loss, float* row_lse, hipStream_t st);
int launch_inbatch_xent_backward(const float* q, const float* c, int B, const float* grad_loss, float* grad_q, float* grad_c, hipStream_t st);

// enc_pooler.hip: pooled = tanh(cls . w_pool^T + b_pool) on [B, 768] rows (HF BertPooler)
int launch_pooler(const float* cls, int64_t B, const float* w_pool, const float* b_pool, float* pooled, hipStream_t st);

}  // namespace aspire
