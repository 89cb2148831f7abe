// A2 + A3: CLS read-out and span mean pooling; A1d's masked token mean (token_mean_pool_kernel, further down).
// Reference: AspireConSent.consent_reps_bert, examples/ex_aspire_consent.py:75-100 -- one full
// [B, L, 768] mask-multiply-sum pass per sentence slot.  Here every token row is read at most once:
// one workgroup of 192 threads per (document, sentence slot); thread t owns the float4 at d = 4t, so a
// token row is a single coalesced 3 KB read; the slot's rows are summed in index order.
// The read-out's backward (what the reference's rank loss sends back to last_hidden_state): span_mean_pool_backward_kernel and
// cls_l2_backward_kernel, each beside its forward.
#include "common.h"

namespace aspire {
namespace {

__global__ void __launch_bounds__(192) span_mean_pool_kernel(const float* __restrict__ hidden, int64_t L,
                                                             const int32_t* __restrict__ tok_idx,
                                                             const int32_t* __restrict__ span_off, int64_t S,
                                                             float* __restrict__ sent_reps,
                                                             float* __restrict__ cls_reps,
                                                             const int32_t* __restrict__ out_row) {
    const int64_t slot = blockIdx.x;          // b * S + s
    const int64_t b = slot / S;
    const int d = threadIdx.x * 4;
    // out_row (rep-store form): slot (b, s) is row out_row[slot] of a rows + CSR store, < 0 = the document has no
    // sentence s (nothing is written: the store holds no padding rows)
    const int64_t orow = out_row != nullptr ? (int64_t)out_row[slot] : slot;
    if (cls_reps != nullptr && slot % S == 0) {
        *reinterpret_cast<float4*>(cls_reps + (size_t)b * kD + d) =
            *reinterpret_cast<const float4*>(hidden + (size_t)b * L * kD + d);
    }
    if (orow < 0) return;
    const float* doc = hidden + (size_t)b * L * kD;
    const int lo = span_off[slot], hi = span_off[slot + 1];
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    int k = lo;
    // 4 rows in flight per thread to cover HBM latency.
    for (; k + 4 <= hi; k += 4) {
        const float4 v0 = ld4_stream(doc + (size_t)tok_idx[k] * kD + d);
        const float4 v1 = ld4_stream(doc + (size_t)tok_idx[k + 1] * kD + d);
        const float4 v2 = ld4_stream(doc + (size_t)tok_idx[k + 2] * kD + d);
        const float4 v3 = ld4_stream(doc + (size_t)tok_idx[k + 3] * kD + d);
        acc.x += v0.x; acc.y += v0.y; acc.z += v0.z; acc.w += v0.w;
        acc.x += v1.x; acc.y += v1.y; acc.z += v1.z; acc.w += v1.w;
        acc.x += v2.x; acc.y += v2.y; acc.z += v2.z; acc.w += v2.w;
        acc.x += v3.x; acc.y += v3.y; acc.z += v3.z; acc.w += v3.w;
    }
    for (; k < hi; ++k) {
        const float4 v = ld4_stream(doc + (size_t)tok_idx[k] * kD + d);
        acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
    }
    // torch.count_nonzero(mask).clamp(min=1): an empty slot stays exactly zero.
    const float cnt = (float)max(hi - lo, 1);
    acc.x /= cnt; acc.y /= cnt; acc.z /= cnt; acc.w /= cnt;
    *reinterpret_cast<float4*>(sent_reps + (size_t)orow * kD + d) = acc;
}

// The gradient of span_mean_pool_kernel with respect to hidden (aspire_span_mean_pool_backward_f32), as a GATHER: one 192-thread
// workgroup per (document, tile of kBwdTile token rows) owns its rows of grad_hidden and is their only writer, so there are no atomics
// and no zero fill in front, and the order of every row's sum is fixed by the walk below, not by the launch.  Thread t owns the
// float4 at d = 4t of every row of the tile (the file's access pattern); the tile lives in LDS because the row a hit lands on is
// only known at run time -- each thread reads and writes its own 16 bytes of each row, so the workgroup needs no barrier.
// The walk: the document's slots in ascending order; a slot's positions 64 at a time, one per lane (every wave of the workgroup walks
// the same list); the lanes whose position lies inside the tile are a ballot, its bits taken from the lowest up = ascending k, each
// a wave-uniform branch.  On a slot's first hit the slot's gradient row is loaded and divided by max(count, 1), once.  A position
// outside [0, L) lies in no tile and is never an address.  The CLS gradient is added last to row 0.  B = 32, L = 256 gives 1024
// workgroups of 24 KB LDS: four per CU.
constexpr int kBwdTile = 8;

__global__ void __launch_bounds__(192) span_mean_pool_backward_kernel(const float* __restrict__ grad_sent,
                                                                      const float* __restrict__ grad_cls, int64_t L, int64_t tiles,
                                                                      const int32_t* __restrict__ tok_idx,
                                                                      const int32_t* __restrict__ span_off, int64_t S,
                                                                      float* __restrict__ grad_hidden) {
    __shared__ float4 tile[kBwdTile][192];
    const int64_t b = blockIdx.x / tiles;
    const int64_t t0 = (blockIdx.x - b * tiles) * kBwdTile;       // the tile: token rows [t0, t0 + rows)
    const int rows = (int)min((int64_t)kBwdTile, L - t0);
    const int th = threadIdx.x, lane = threadIdx.x & 63;
#pragma unroll
    for (int r = 0; r < kBwdTile; ++r) tile[r][th] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (grad_sent != nullptr) {
        for (int64_t s = 0; s < S; ++s) {
            const int lo = span_off[b * S + s], hi = span_off[b * S + s + 1];
            bool have = false;
            float4 g = make_float4(0.f, 0.f, 0.f, 0.f);
            for (int k0 = lo; k0 < hi; k0 += 64) {
                const int k = k0 + lane;
                const int64_t rel = k < hi ? (int64_t)tok_idx[k] - t0 : -1;
                const bool hit = rel >= 0 && rel < rows;
                unsigned long long todo = __ballot(hit);
                while (todo != 0) {
                    const int src = __ffsll(todo) - 1;
                    todo &= todo - 1;
                    const int r = __shfl((int)rel, src);
                    if (!have) {
                        have = true;
                        g = *reinterpret_cast<const float4*>(grad_sent + (size_t)(b * S + s) * kD + th * 4);
                        const float cnt = (float)max(hi - lo, 1);
                        g.x /= cnt; g.y /= cnt; g.z /= cnt; g.w /= cnt;
                    }
                    float4 a = tile[r][th];
                    a.x += g.x; a.y += g.y; a.z += g.z; a.w += g.w;
                    tile[r][th] = a;
                }
            }
        }
    }
    if (grad_cls != nullptr && t0 == 0) {
        const float4 c = *reinterpret_cast<const float4*>(grad_cls + (size_t)b * kD + th * 4);
        float4 a = tile[0][th];
        a.x += c.x; a.y += c.y; a.z += c.z; a.w += c.w;
        tile[0][th] = a;
    }
    float* dst = grad_hidden + ((size_t)b * L + (size_t)t0) * kD + th * 4;
    for (int r = 0; r < rows; ++r) *reinterpret_cast<float4*>(dst + (size_t)r * kD) = tile[r][th];
}

// Ragged span pooling (aspire_span_pool_ranges_f32): every output row is a RANGE of token rows of one document, so the grid is over
// the rows that exist and no token-index list is read.  One 192-thread workgroup per output row, thread t owns the float4 at d = 4t
// (span_mean_pool_kernel's access pattern: a token row is one coalesced 3 KB read), but 16 token rows in flight per thread instead
// of 4: the kernel's time is the LONGEST span's chain of dependent load rounds (a row's sum keeps the token order, so a span is
// not split over workgroups), and every entity span (1 - 6 tokens) and most sentence spans are a single round.  (One wave per row
// with three float4s per lane, four rows per workgroup, was measured first: 38 us where span_mean_pool_kernel takes 28 us on the
// same spans -- a wave holds a quarter of the loads in flight per token row)  The sum runs in ascending
// token order and is divided by max(tok_len, 1): the same bits as span_mean_pool_kernel on the same span.
// Workgroups beyond the R row blocks copy the CLS rows, one document each.
constexpr int kRangeDepth = 16;

__global__ void __launch_bounds__(192) span_pool_ranges_kernel(const float* __restrict__ hidden, int64_t B, int64_t L,
                                                               const int32_t* __restrict__ row_doc,
                                                               const int32_t* __restrict__ row_start,
                                                               const int32_t* __restrict__ row_len, int64_t R,
                                                               const int32_t* __restrict__ out_row, float* __restrict__ rows,
                                                               float* __restrict__ cls_reps) {
    const int d = threadIdx.x * 4;
    const int64_t r = blockIdx.x;
    if (r >= R) {
        const int64_t b = r - R;
        if (cls_reps == nullptr || b >= B) return;
        *reinterpret_cast<float4*>(cls_reps + (size_t)b * kD + d) =
            *reinterpret_cast<const float4*>(hidden + (size_t)b * L * kD + d);
        return;
    }
    const int64_t orow = out_row != nullptr ? (int64_t)out_row[r] : r;
    const int n = row_len[r];
    const float* src = hidden + ((size_t)row_doc[r] * L + (size_t)row_start[r]) * kD + d;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    int t = 0;
    for (; t + kRangeDepth <= n; t += kRangeDepth) {
        float4 v[kRangeDepth];
#pragma unroll
        for (int u = 0; u < kRangeDepth; ++u) v[u] = ld4_stream(src + (size_t)(t + u) * kD);
#pragma unroll
        for (int u = 0; u < kRangeDepth; ++u) {
            acc.x += v[u].x; acc.y += v[u].y; acc.z += v[u].z; acc.w += v[u].w;
        }
    }
    for (; t + 4 <= n; t += 4) {
        float4 v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) v[u] = ld4_stream(src + (size_t)(t + u) * kD);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            acc.x += v[u].x; acc.y += v[u].y; acc.z += v[u].z; acc.w += v[u].w;
        }
    }
    for (; t < n; ++t) {
        const float4 v = ld4_stream(src + (size_t)t * kD);
        acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
    }
    // an empty span stays exactly zero (span_mean_pool_kernel's empty-slot rule)
    const float cnt = (float)max(n, 1);
    acc.x /= cnt; acc.y /= cnt; acc.z /= cnt; acc.w /= cnt;
    *reinterpret_cast<float4*>(rows + (size_t)orow * kD + d) = acc;
}

// A1d's read-out: sentence-transformers' Pooling in mean mode and its Normalize module (SentenceModel.encode,
// src/evaluation/utils/models.py:392-406, through SentenceTransformer.encode).  One 192-thread workgroup per sentence, thread t owns
// the float4 at d = 4t as above; the token rows with mask != 0 are summed in token order, eight in flight per thread, rows of masked
// tokens are never read (the mask words are the same for the whole workgroup: the skip is a uniform branch).  Then / max(count, 1e-9)
// (torch.clamp(sum_mask, min=1e-9)) and, with normalize, / max(||x||_2, 1e-12) (F.normalize): the 768 squares summed per thread, per
// wave and over the three waves through LDS.  A sentence without a valid token gives exact zeros (0 / 1e-9, then 0 / 1e-12).
__global__ void __launch_bounds__(192) token_mean_pool_kernel(const float* __restrict__ hidden, const int64_t* __restrict__ mask, int64_t L,
                                                              int normalize, float* __restrict__ out) {
    __shared__ float part[3];
    const int64_t b = blockIdx.x;
    const int d = threadIdx.x * 4;
    const float* src = hidden + (size_t)b * L * kD + d;
    const int64_t* mk = mask + b * L;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    int count = 0;
    for (int64_t t = 0; t < L; t += 8) {
        float4 v[8];
        bool on[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            on[u] = t + u < L && mk[min(t + u, L - 1)] != 0;
            if (on[u]) v[u] = ld4_stream(src + (size_t)(t + u) * kD);
        }
#pragma unroll
        for (int u = 0; u < 8; ++u)
            if (on[u]) {
                acc.x += v[u].x; acc.y += v[u].y; acc.z += v[u].z; acc.w += v[u].w;
                ++count;
            }
    }
    const float cnt = fmaxf((float)count, 1e-9f);
    acc.x /= cnt; acc.y /= cnt; acc.z /= cnt; acc.w /= cnt;
    if (normalize) {
        const float q = wave_sum((acc.x * acc.x + acc.y * acc.y) + (acc.z * acc.z + acc.w * acc.w));
        if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = q;
        __syncthreads();
        const float nrm = fmaxf(sqrtf((part[0] + part[1]) + part[2]), 1e-12f);
        acc.x /= nrm; acc.y /= nrm; acc.z /= nrm; acc.w /= nrm;
    }
    *reinterpret_cast<float4*>(out + (size_t)b * kD + d) = acc;
}

// caching_score's document-level term: ||q_cls - c_cls + eps||_2 (torch.nn.functional.pairwise_distance), one wave per
// pair, 12 coordinates per lane.
__global__ void __launch_bounds__(256) cls_l2_kernel(const float* __restrict__ q_cls, int64_t Q, const float* __restrict__ c_cls,
                                                     int64_t C, int paired, float eps, float* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int64_t pair = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int64_t P = paired ? C : Q * C;
    if (pair >= P) return;
    const int64_t qi = paired ? pair : pair / C, ci = paired ? pair : pair - qi * C;
    const float* x = q_cls + (size_t)qi * kD + lane * 4;
    const float* y = c_cls + (size_t)ci * kD + lane * 4;
    float acc = 0.f;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float4 u = *reinterpret_cast<const float4*>(x + 256 * k), v = *reinterpret_cast<const float4*>(y + 256 * k);
        const float d0 = (u.x - v.x) + eps, d1 = (u.y - v.y) + eps, d2 = (u.z - v.z) + eps, d3 = (u.w - v.w) + eps;
        acc = fmaf(d3, d3, fmaf(d2, d2, fmaf(d1, d1, fmaf(d0, d0, acc))));
    }
    acc = wave_sum(acc);
    if (lane == 0) out[pair] = sqrtf(acc);
}

// Its gradient for paired rows (aspire_cls_l2_backward_f32): one wave per pair, the distance formed again exactly as above (the same
// differences, the same fma chain, the same wave sum), then grad_q = (q - c + eps) * (g / dist), grad_c = -grad_q: torch's rule for
// the 2-norm, zeros where dist == 0.  Each lane writes the 12 coordinates it read.
__global__ void __launch_bounds__(256) cls_l2_backward_kernel(const float* __restrict__ q_cls, const float* __restrict__ c_cls, int64_t P,
                                                              float eps, const float* __restrict__ grad_dist, float* __restrict__ grad_q,
                                                              float* __restrict__ grad_c) {
    const int lane = threadIdx.x & 63;
    const int64_t pair = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (pair >= P) return;
    const size_t at = (size_t)pair * kD + lane * 4;
    float4 d[3];
    float acc = 0.f;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float4 u = *reinterpret_cast<const float4*>(q_cls + at + 256 * k), v = *reinterpret_cast<const float4*>(c_cls + at + 256 * k);
        d[k] = make_float4((u.x - v.x) + eps, (u.y - v.y) + eps, (u.z - v.z) + eps, (u.w - v.w) + eps);
        acc = fmaf(d[k].w, d[k].w, fmaf(d[k].z, d[k].z, fmaf(d[k].y, d[k].y, fmaf(d[k].x, d[k].x, acc))));
    }
    const float dist = sqrtf(wave_sum(acc));
    const float r = dist > 0.f ? grad_dist[pair] / dist : 0.f;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float4 g = make_float4(d[k].x * r, d[k].y * r, d[k].z * r, d[k].w * r);
        *reinterpret_cast<float4*>(grad_q + at + 256 * k) = g;
        *reinterpret_cast<float4*>(grad_c + at + 256 * k) = make_float4(-g.x, -g.y, -g.z, -g.w);
    }
}

}  // namespace
}  // namespace aspire

using namespace aspire;

extern "C" int aspire_cls_l2_f32(const float* q_cls, int64_t Q, const float* c_cls, int64_t C, int64_t D, int pairing, double eps,
                                 float* dist, void* stream) {
    ASPIRE_REQUIRE(D == kD, ASPIRE_ERR_UNSUPPORTED, "encoding dim %lld unsupported (kernels are built for 768)", (long long)D);
    ASPIRE_REQUIRE(pairing == ASPIRE_PAIR_CROSS || pairing == ASPIRE_PAIR_PAIRED, ASPIRE_ERR_INVALID_ARG, "bad pairing %d", pairing);
    ASPIRE_REQUIRE(Q >= 0 && C >= 0 && (pairing != ASPIRE_PAIR_PAIRED || Q == C), ASPIRE_ERR_INVALID_ARG,
                   "paired distances need equal batch sizes (query %lld vs cand %lld)", (long long)Q, (long long)C);
    const int64_t P = pairing == ASPIRE_PAIR_PAIRED ? C : Q * C;
    if (P == 0) return ASPIRE_OK;
    ASPIRE_REQUIRE(q_cls && c_cls && dist, ASPIRE_ERR_INVALID_ARG, "null pointer");
    hipLaunchKernelGGL(cls_l2_kernel, dim3((unsigned)((P + 3) / 4)), dim3(256), 0, (hipStream_t)stream, q_cls, Q, c_cls, C,
                       pairing == ASPIRE_PAIR_PAIRED ? 1 : 0, (float)eps, dist);
    ASPIRE_LAUNCH_OK();
    return ASPIRE_OK;
}

extern "C" int aspire_cls_l2_backward_f32(const float* q_cls, int64_t Q, const float* c_cls, int64_t C, int64_t D, int pairing, double eps,
                                          const float* grad_dist, float* grad_q, float* grad_c, void* stream) {
    ASPIRE_REQUIRE(D == kD, ASPIRE_ERR_UNSUPPORTED, "encoding dim %lld unsupported (kernels are built for 768)", (long long)D);
    ASPIRE_REQUIRE(pairing == ASPIRE_PAIR_CROSS || pairing == ASPIRE_PAIR_PAIRED, ASPIRE_ERR_INVALID_ARG, "bad pairing %d", pairing);
    ASPIRE_REQUIRE(pairing == ASPIRE_PAIR_PAIRED, ASPIRE_ERR_UNSUPPORTED,
                   "the backward is built for ASPIRE_PAIR_PAIRED only (ASPIRE_PAIR_CROSS needs an accumulation across pairs)");
    ASPIRE_REQUIRE(Q >= 0 && Q == C, ASPIRE_ERR_INVALID_ARG, "paired distances need equal batch sizes (query %lld vs cand %lld)",
                   (long long)Q, (long long)C);
    if (C == 0) return ASPIRE_OK;
    ASPIRE_REQUIRE(q_cls && c_cls && grad_dist && grad_q && grad_c, ASPIRE_ERR_INVALID_ARG, "null pointer");
    ASPIRE_REQUIRE((((uintptr_t)q_cls | (uintptr_t)c_cls | (uintptr_t)grad_q | (uintptr_t)grad_c) & 15) == 0, ASPIRE_ERR_INVALID_ARG,
                   "the CLS rows and their gradients must be 16-byte aligned");
    hipLaunchKernelGGL(cls_l2_backward_kernel, dim3((unsigned)((C + 3) / 4)), dim3(256), 0, (hipStream_t)stream, q_cls, c_cls, C,
                       (float)eps, grad_dist, grad_q, grad_c);
    ASPIRE_LAUNCH_OK();
    return ASPIRE_OK;
}

extern "C" int aspire_span_mean_pool_backward_f32(const float* grad_sent, const float* grad_cls, int64_t B, int64_t L, int64_t D,
                                                  const int32_t* tok_idx, const int32_t* span_off, int64_t S, float* grad_hidden,
                                                  void* stream) {
    ASPIRE_REQUIRE(D == kD, ASPIRE_ERR_UNSUPPORTED, "encoding dim %lld unsupported (kernels are built for 768)", (long long)D);
    ASPIRE_REQUIRE(B >= 0 && L >= 0 && S > 0, ASPIRE_ERR_INVALID_ARG, "bad shape B=%lld L=%lld S=%lld", (long long)B, (long long)L,
                   (long long)S);
    if (B == 0 || L == 0) return ASPIRE_OK;
    ASPIRE_REQUIRE(grad_hidden && (grad_sent == nullptr || span_off), ASPIRE_ERR_INVALID_ARG, "null pointer");
    ASPIRE_REQUIRE((((uintptr_t)grad_sent | (uintptr_t)grad_cls | (uintptr_t)grad_hidden) & 15) == 0, ASPIRE_ERR_INVALID_ARG,
                   "the gradients must be 16-byte aligned");
    const int64_t tiles = (L + kBwdTile - 1) / kBwdTile;
    ASPIRE_REQUIRE(B <= 0x7fffffffLL / tiles, ASPIRE_ERR_UNSUPPORTED, "%lld documents of %lld tokens in one call", (long long)B,
                   (long long)L);
    hipLaunchKernelGGL(span_mean_pool_backward_kernel, dim3((unsigned)(B * tiles)), dim3(192), 0, (hipStream_t)stream, grad_sent,
                       grad_cls, L, tiles, tok_idx, span_off, S, grad_hidden);
    ASPIRE_LAUNCH_OK();
    return ASPIRE_OK;
}

extern "C" int aspire_span_mean_pool_f32(const float* hidden, int64_t B, int64_t L, int64_t D, const int32_t* tok_idx,
                                         const int32_t* span_off, int64_t S, float* sent_reps, float* cls_reps,
                                         void* stream) {
    ASPIRE_REQUIRE(D == kD, ASPIRE_ERR_UNSUPPORTED, "encoding dim %lld unsupported (kernels are built for 768)",
                   (long long)D);
    ASPIRE_REQUIRE(B >= 0 && L > 0 && S > 0, ASPIRE_ERR_INVALID_ARG, "bad shape B=%lld L=%lld S=%lld", (long long)B,
                   (long long)L, (long long)S);
    ASPIRE_REQUIRE(hidden && span_off && sent_reps, ASPIRE_ERR_INVALID_ARG, "null pointer");
    if (B == 0) return ASPIRE_OK;
    hipLaunchKernelGGL(span_mean_pool_kernel, dim3((unsigned)(B * S)), dim3(192), 0, (hipStream_t)stream, hidden, L,
                       tok_idx, span_off, S, sent_reps, cls_reps, (const int32_t*)nullptr);
    ASPIRE_LAUNCH_OK();
    return ASPIRE_OK;
}

extern "C" int aspire_span_mean_pool_rows_f32(const float* hidden, int64_t B, int64_t L, int64_t D, const int32_t* tok_idx,
                                              const int32_t* span_off, int64_t S, const int32_t* out_row, float* rows,
                                              float* cls_reps, void* stream) {
    ASPIRE_REQUIRE(D == kD, ASPIRE_ERR_UNSUPPORTED, "encoding dim %lld unsupported (kernels are built for 768)",
                   (long long)D);
    ASPIRE_REQUIRE(B >= 0 && L > 0 && S > 0, ASPIRE_ERR_INVALID_ARG, "bad shape B=%lld L=%lld S=%lld", (long long)B,
                   (long long)L, (long long)S);
    ASPIRE_REQUIRE(hidden && span_off && out_row && rows, ASPIRE_ERR_INVALID_ARG, "null pointer");
    if (B == 0) return ASPIRE_OK;
    hipLaunchKernelGGL(span_mean_pool_kernel, dim3((unsigned)(B * S)), dim3(192), 0, (hipStream_t)stream, hidden, L,
                       tok_idx, span_off, S, rows, cls_reps, out_row);
    ASPIRE_LAUNCH_OK();
    return ASPIRE_OK;
}

extern "C" int aspire_span_pool_ranges_f32(const float* hidden, int64_t B, int64_t L, int64_t D, const int32_t* row_doc,
                                           const int32_t* row_start, const int32_t* row_len, int64_t R, const int32_t* out_row,
                                           float* rows, float* cls_reps, void* stream) {
    ASPIRE_REQUIRE(D == kD, ASPIRE_ERR_UNSUPPORTED, "encoding dim %lld unsupported (kernels are built for 768)",
                   (long long)D);
    ASPIRE_REQUIRE(B >= 0 && L > 0 && R >= 0, ASPIRE_ERR_INVALID_ARG, "bad shape B=%lld L=%lld R=%lld", (long long)B,
                   (long long)L, (long long)R);
    ASPIRE_REQUIRE(hidden || B == 0, ASPIRE_ERR_INVALID_ARG, "null pointer");
    ASPIRE_REQUIRE(R == 0 || (row_doc && row_start && row_len && rows), ASPIRE_ERR_INVALID_ARG, "null pointer");
    ASPIRE_REQUIRE(R == 0 || B > 0, ASPIRE_ERR_INVALID_ARG, "%lld rows of a batch without documents", (long long)R);
    const int64_t row_blocks = R;
    const int64_t cls_blocks = cls_reps != nullptr ? B : 0;
    if (row_blocks + cls_blocks == 0) return ASPIRE_OK;
    ASPIRE_REQUIRE(row_blocks + cls_blocks <= 0x7fffffffLL, ASPIRE_ERR_UNSUPPORTED, "%lld rows in one call", (long long)R);
    hipLaunchKernelGGL(span_pool_ranges_kernel, dim3((unsigned)(row_blocks + cls_blocks)), dim3(192), 0, (hipStream_t)stream,
                       hidden, B, L, row_doc, row_start, row_len, R, out_row, rows, cls_reps);
    ASPIRE_LAUNCH_OK();
    return ASPIRE_OK;
}

extern "C" int aspire_token_mean_pool_f32(const float* hidden, const int64_t* attn_mask, int64_t B, int64_t L, int64_t D, int normalize,
                                          float* out, void* stream) {
    ASPIRE_REQUIRE(D == kD, ASPIRE_ERR_UNSUPPORTED, "encoding dim %lld unsupported (kernels are built for 768)", (long long)D);
    ASPIRE_REQUIRE(B >= 0 && L > 0, ASPIRE_ERR_INVALID_ARG, "bad shape B=%lld L=%lld", (long long)B, (long long)L);
    if (B == 0) return ASPIRE_OK;
    ASPIRE_REQUIRE(hidden && attn_mask && out, ASPIRE_ERR_INVALID_ARG, "null pointer");
    ASPIRE_REQUIRE(((uintptr_t)hidden & 15) == 0 && ((uintptr_t)out & 15) == 0, ASPIRE_ERR_INVALID_ARG,
                   "hidden and out must be 16-byte aligned");
    ASPIRE_REQUIRE(B <= 0x7fffffffLL, ASPIRE_ERR_UNSUPPORTED, "%lld sentences in one call", (long long)B);
    hipLaunchKernelGGL(token_mean_pool_kernel, dim3((unsigned)B), dim3(192), 0, (hipStream_t)stream, hidden, attn_mask, L, normalize, out);
    ASPIRE_LAUNCH_OK();
    return ASPIRE_OK;
}
