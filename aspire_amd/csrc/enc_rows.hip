// The encoder's row-wise kernels: one wave per row of 768, four rows per workgroup.
//
// Kernels
//   layernorm_kernel         y = LN(x) * gamma + beta, eps 1e-12; optionally also into the P layout (enc_planes.h)  (one wave per token)
//   embed_layernorm_kernel   word + position + token-type gather, LayerNorm; same outputs                          (one wave per token)
//                            the position row is the token's index (BertModel) or pos_ids[token] (RoBERTa / MPNet: aspire_bert_extras)
//   cls_tap_kernel           the CLS row of every document of a hidden state (fp32 or planes) -> layer_cls, the layer mix, the last
//                            layer's residual input (aspire_bert_forward_cls_f32)                                   (one wave per document)
#include "enc_planes.h"
#include "enc_types.h"

namespace aspire {
namespace {

// One wave per row of 768: lane holds 3 float4 (d = 4*lane + 256*c).
// yp (optional): the row also goes out in the P layout (rows = `rows`), the A operand of the GEMM that reads it
__device__ __forceinline__ void layernorm_row(float4 (&v)[3], const float* gamma, const float* beta, float eps,
                                              float* out, int lane, void* yp = nullptr, int64_t rows = 0, int64_t row = 0) {
    float s = 0.f;
#pragma unroll
    for (int c = 0; c < 3; ++c) s += (v[c].x + v[c].y) + (v[c].z + v[c].w);
    const float mean = wave_sum(s) * (1.0f / kD);
    float q = 0.f;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float a = v[c].x - mean, b = v[c].y - mean, cc = v[c].z - mean, d = v[c].w - mean;
        q += (a * a + b * b) + (cc * cc + d * d);
    }
    const float rstd = 1.0f / sqrtf(wave_sum(q) * (1.0f / kD) + eps);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const int d = 4 * lane + 256 * c;
        const float4 gm = *reinterpret_cast<const float4*>(gamma + d), bt = *reinterpret_cast<const float4*>(beta + d);
        float4 o;
        o.x = (v[c].x - mean) * rstd * gm.x + bt.x;
        o.y = (v[c].y - mean) * rstd * gm.y + bt.y;
        o.z = (v[c].z - mean) * rstd * gm.z + bt.z;
        o.w = (v[c].w - mean) * rstd * gm.w + bt.w;
        *reinterpret_cast<float4*>(out + d) = o;
        if (yp) p_store4(yp, rows, row, d, o.x, o.y, o.z, o.w);
    }
}

__global__ void __launch_bounds__(256) layernorm_kernel(const float* __restrict__ x, const float* __restrict__ gamma,
                                                        const float* __restrict__ beta, float eps, float* __restrict__ y,
                                                        int64_t rows, void* __restrict__ yp) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    float4 v[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c] = *reinterpret_cast<const float4*>(x + row * kD + 4 * lane + 256 * c);
    layernorm_row(v, gamma, beta, eps, y + row * kD, lane, yp, rows, row);
}

__global__ void __launch_bounds__(256) embed_layernorm_kernel(const int64_t* __restrict__ tok, const int64_t* __restrict__ typ,
                                                              const int64_t* __restrict__ pos_ids, const float* __restrict__ word, const float* __restrict__ pos,
                                                              const float* __restrict__ type_emb, const float* __restrict__ gamma,
                                                              const float* __restrict__ beta, float eps, float* __restrict__ y,
                                                              int64_t rows, int64_t L, void* __restrict__ yp) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int64_t t = tok[row], ty = typ ? typ[row] : 0, p = pos_ids ? pos_ids[row] : row % L;
    float4 v[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const int d = 4 * lane + 256 * c;
        const float4 a = *reinterpret_cast<const float4*>(word + t * kD + d);
        const float4 b = *reinterpret_cast<const float4*>(type_emb + ty * kD + d);
        const float4 e = *reinterpret_cast<const float4*>(pos + p * kD + d);
        // BertEmbeddings / RobertaEmbeddings: inputs_embeds + token_type_embeddings, then + position_embeddings (MPNet has no token
        // types: its one type row is zero, and (a + 0) + e = a + e)
        v[c] = make_float4((a.x + b.x) + e.x, (a.y + b.y) + e.y, (a.z + b.z) + e.z, (a.w + b.w) + e.w);
    }
    layernorm_row(v, gamma, beta, eps, y + row * kD, lane, yp, rows, row);
}

// The CLS row (row b L) of each of the B documents of one hidden state, read from fp32 x [rows, 768] or from the P-layout planes xp
// (the fused-LayerNorm form's actp: p_slot, as the GEMMs that write it): -> layer_cls [B, 768] and gather [B, 768] (each optional);
// mode 1: cls_out = wt x row, 2: cls_out += wt x row, 0: cls_out untouched.  One wave per document.
__global__ void __launch_bounds__(256) cls_tap_kernel(const float* __restrict__ x, const void* __restrict__ xp, int64_t rows, int64_t L,
                                                      int64_t B, float wt, int mode, float* __restrict__ cls_out,
                                                      float* __restrict__ layer_cls, float* __restrict__ gather) {
    const int lane = threadIdx.x & 63;
    const int64_t b = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= B) return;
    const int64_t r = b * L;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const int d = 4 * lane + 256 * c;
        const float4 v = xp ? p_load4_at(xp, p_slot((uint32_t)rows, (uint32_t)r, (uint32_t)d)) : *reinterpret_cast<const float4*>(x + r * kD + d);
        const size_t o = (size_t)b * kD + d;
        if (layer_cls) *reinterpret_cast<float4*>(layer_cls + o) = v;
        if (gather) *reinterpret_cast<float4*>(gather + o) = v;
        if (mode) {
            float4 a = make_float4(wt * v.x, wt * v.y, wt * v.z, wt * v.w);
            if (mode == 2) {
                const float4 p = *reinterpret_cast<const float4*>(cls_out + o);
                a = make_float4(p.x + a.x, p.y + a.y, p.z + a.z, p.w + a.w);
            }
            *reinterpret_cast<float4*>(cls_out + o) = a;
        }
    }
}

}  // namespace

int launch_layernorm(const float* x, const float* gamma, const float* beta, float eps, float* y, int64_t rows, void* yp, hipStream_t st) {
    hipLaunchKernelGGL(layernorm_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, st, x, gamma, beta, eps, y, rows, yp);
    ASPIRE_LAUNCH_OK();
    return ASPIRE_OK;
}

int launch_embed_layernorm(const int64_t* tok, const int64_t* typ, const int64_t* pos_ids, const float* word, const float* pos,
                           const float* type_emb, const float* gamma, const float* beta, float eps, float* y, int64_t rows, int64_t L,
                           void* yp, hipStream_t st) {
    hipLaunchKernelGGL(embed_layernorm_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, st, tok, typ, pos_ids, word, pos, type_emb,
                       gamma, beta, eps, y, rows, L, yp);
    ASPIRE_LAUNCH_OK();
    return ASPIRE_OK;
}

int launch_cls_tap(const float* x, const void* xp, int64_t rows, int64_t L, int64_t B, float wt, int mode, float* cls_out, float* layer_cls,
                   float* gather, hipStream_t st) {
    hipLaunchKernelGGL(cls_tap_kernel, dim3((unsigned)((B + 3) / 4)), dim3(256), 0, st, x, xp, rows, L, B, wt, mode, cls_out, layer_cls, gather);
    ASPIRE_LAUNCH_OK();
    return ASPIRE_OK;
}

}  // namespace aspire
