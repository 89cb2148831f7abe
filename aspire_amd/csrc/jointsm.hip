// Joint soft-max sentence alignment: the 'jointsm' score of WordSentAlignPolyEnc (include/aspire_hip.h, A14).
//
//   d_ij  = <q_i, c_j>                                   torch.bmm (pair_distances.py:371)
//   p     = softmax over ALL valid (i < q_len, j < c_len) jointly of d_ij / sqrt(768)
//                                                        (pair_distances.py:372-373, activations.py:35-61: -1e32 outside the block,
//                                                        log_softmax(...).exp() over the flattened block: pads come out exactly 0)
//   score = sum_i <q_i, sum_j p_ij c_j> + sum_j <c_j, sum_i p_ij q_i> = 2 sum_ij p_ij d_ij      (pair_distances.py:376-397)
//
// The dot products are formed as dotmax.hip forms them (dot_tiles.h: exact fp32 on v_mfma_f32_16x16x4_f32, the same operand
// layout and eight-k step, the same bits in both kernels of this file), but over SIXTEEN accumulators per tile instead of four:
// k block s goes to accumulator set s & 3, so a chain is 48 fmaf long, not 192, and its partial sums a sixteenth of the dot.
// Sentence rows share a large common component, their products are mostly of one sign, and a four-chain sum of a 1 x 1 pair sits
// 2.7e-7 (relative) from float64 where the reference's own sgemm sits at 1e-7: the parity bar (twice the reference's error) needs
// the shorter chains; sixteen give 6e-8.  The registers are there (one wave per SIMD in the cross kernel, two in the pair kernel).
// The [rows_q, rows_c] block is never written unless pair_softmax is asked for.  The epilogue keeps the
// soft-max shifted by the running maximum m of the RAW dots (the scaling is monotonic) and sums, beside S = sum e_ij with
// e_ij = exp((d_ij - m) / sqrtf(768)), the CENTRED T = sum e_ij (d_ij - m):
//   score = 2 (m + T / S)
// Scores are large (hundreds to thousands) and the logits reach +-70: the shift happens before the division, so the exponent's
// argument carries the rounding of a small number, and T / S is a correction of a few sqrt(768) to m, so the rounding of the two
// long sums reaches the score scaled down by that ratio.  A new maximum m' rescales with f = exp((m - m') / sqrtf(768)):
// S <- f S, T <- f (T + (m - m') S).
//   jointsm_pair_kernel   one wave per (query, candidate) pair, 16 x 16 tiles over documents of up to 128 rows, m wave-uniform
//                         (one wave_max per tile), S and T per lane until the end: PAIRED, the jobs of
//                         aspire_jointsm_rank_batch_f32, CROSS with longer documents, and every call that wants pair_softmax
//                         (pass 1 leaves d_ij in the output block, pass 2 -- every lane over its own entries -- turns them
//                         into p_ij once m and S are final, then the pad entries are zeroed).
//   jointsm_cross_kernel  CROSS with documents of <= 16 rows: dotmax_cross_kernel's layout (32 candidate row slots per workgroup in
//                         LDS, the query rows streamed in chunks of 16 slots); max, S and T are segmented all-reductions over the
//                         W_q lanes x W_c rows of a document pair.
// The two kernels sum S and T in different orders: a pair's score agrees between them to rounding, not
// in every bit.
#include <math.h>

#include "common.h"
#include "batch_host.h"
#include "dot_tiles.h"

namespace aspire {
namespace {

struct JsmArgs {
    DotSet q, c;
    int mode;
    const int32_t* job_off;     // kModeMapped: [J + 1]
    int32_t J;
    int32_t wq_log, wc_log;     // cross kernel: log2 of the row slots per document
    float* scores;
    float* pair_softmax;        // pair kernel, padded sets: [P, q.bound, c.bound], or null
};

// exp((d - m) / sqrt(encoding_dim)) for d <= m: torch.div(pair_sims, math.sqrt(encoding_dim)) behind the max shift
__device__ __forceinline__ float shifted_exp(float y) { return expf(y / sqrtf((float)kD)); }

// ---- one wave per pair --------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) jointsm_pair_kernel(JsmArgs a, int64_t P) {
    const int lane = threadIdx.x & 63, g = lane >> 4, r = lane & 15;
    const int64_t p = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (p >= P) return;
    int64_t qi, ci;
    if (a.mode == kModeCross) {
        qi = p / a.c.n;
        ci = p - qi * a.c.n;
    } else if (a.mode == kModePaired) {
        qi = ci = p;
    } else {
        ci = p;
        qi = job_of(a.job_off, a.J, p);
    }
    const int ql = a.q.len[qi], cl = a.c.len[ci];
    const int qext = a.q.bound, cext = a.c.bound;
    float* soft = a.pair_softmax ? a.pair_softmax + p * qext * cext : nullptr;
    if (ql > qext || cl > cext) {
        if (lane == 0) a.scores[p] = __builtin_nanf("");
        if (soft)
            for (int e = lane; e < qext * cext; e += 64) soft[e] = __builtin_nanf("");
        return;
    }
    const float* qbase = a.q.rows + (int64_t)a.q.start[qi] * kD + 8 * g;
    const float* cbase = a.c.rows + (int64_t)a.c.start[ci] * kD + 8 * g;
    float m = -INFINITY, S = 0.f, T = 0.f;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    for (int c0 = 0; c0 < cl; c0 += 16) {
        const bool va = c0 + r < cl;
        const float* pa = cbase + (int64_t)(va ? c0 + r : 0) * kD;
        for (int q0 = 0; q0 < ql; q0 += 16) {
            const bool vb = q0 + r < ql;
            const float* pb = qbase + (int64_t)(vb ? q0 + r : 0) * kD;
            f32x4 acc[4][4] = {{zero, zero, zero, zero}, {zero, zero, zero, zero}, {zero, zero, zero, zero}, {zero, zero, zero, zero}};
            for (int s0 = 0; s0 < kD / 32; s0 += 4) {
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int s = s0 + u;
                    const f32x4 a0 = va ? ld4(pa + 32 * s) : zero, a1 = va ? ld4(pa + 32 * s + 4) : zero;
                    const f32x4 b0 = vb ? ld4(pb + 32 * s) : zero, b1 = vb ? ld4(pb + 32 * s + 4) : zero;
                    mfma8(a0, a1, b0, b1, acc[u]);
                }
            }
            // C[row 4 g + v][col r]: candidate row c0 + 4 g + v, query row q0 + r
            const f32x4 dot = tile_dots(acc);
            float tile_max = -INFINITY;
#pragma unroll
            for (int v = 0; v < 4; ++v)
                if (c0 + 4 * g + v < cl && vb) tile_max = fmaxf(tile_max, dot[v]);
            tile_max = wave_max(tile_max);
            if (tile_max > m) {                 // wave-uniform
                if (m > -INFINITY) {
                    const float dm = m - tile_max, f = shifted_exp(dm);
                    T = f * fmaf(dm, S, T);
                    S = f * S;
                }
                m = tile_max;
            }
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                if (c0 + 4 * g + v < cl && vb) {
                    const float y = dot[v] - m, e = shifted_exp(y);
                    S += e;
                    T = fmaf(e, y, T);
                    if (soft) soft[(q0 + r) * cext + c0 + 4 * g + v] = dot[v];
                }
            }
        }
    }
    S = wave_sum(S);
    T = wave_sum(T);
    if (lane == 0) a.scores[p] = 2.0f * (m + T / S);
    if (!soft) return;
    // every lane turns the dots it left in the block into p_ij (its own stores: program order), then the pads are zeroed
    for (int c0 = 0; c0 < cl; c0 += 16) {
        for (int q0 = 0; q0 < ql; q0 += 16) {
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                if (c0 + 4 * g + v < cl && q0 + r < ql) {
                    float* at = soft + (q0 + r) * cext + c0 + 4 * g + v;
                    *at = shifted_exp(*at - m) / S;
                }
            }
        }
    }
    for (int e = lane; e < qext * cext; e += 64) {
        const int i = e / cext, j = e - i * cext;
        if (i >= ql || j >= cl) soft[e] = 0.0f;
    }
}

// ---- CROSS, documents of <= 16 rows: 32 candidate row slots per workgroup in LDS --------------------------------------
// all-reduce over one document pair's entries of a 16 x 16 tile: the query document's rows sit on Wq neighbouring lanes, the
// candidate document's Wc rows on registers v, then lane groups g
template <typename Op>
__device__ __forceinline__ void pair_block_allreduce(float (&m)[4], int Wq, int Wc, Op op) {
#pragma unroll
    for (int v = 0; v < 4; ++v)
        for (int sh = 1; sh < Wq; sh <<= 1) m[v] = op(m[v], __shfl_xor(m[v], sh));
    if (Wc >= 2) {
        m[0] = m[1] = op(m[0], m[1]);
        m[2] = m[3] = op(m[2], m[3]);
    }
    if (Wc >= 4) m[0] = m[1] = m[2] = m[3] = op(m[0], m[2]);
    if (Wc >= 8) {
        m[0] = op(m[0], __shfl_xor(m[0], 16));
        if (Wc >= 16) m[0] = op(m[0], __shfl_xor(m[0], 32));
        m[1] = m[2] = m[3] = m[0];
    }
}

__global__ void __launch_bounds__(256) jointsm_cross_kernel(JsmArgs a) {
    __shared__ __attribute__((aligned(16))) float As[kXRows * kXStride];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, r = lane & 15;
    const int Wc = 1 << a.wc_log, Wq = 1 << a.wq_log;
    const int64_t C = a.c.n, Q = a.q.n;
    const int64_t slot0 = (int64_t)blockIdx.x * kXRows;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    // stage: four threads per row slot (waves 0 and 1), thread g reads k = 32 s + 8 g .. + 7 -- the k values lane group g of
    // jointsm_pair_kernel reads, so the two kernels form the same dot products bit for bit
    if (tid < 4 * kXRows) {
        const int R = tid >> 2, gs = tid & 3;
        const int64_t vrow = slot0 + R, doc = vrow >> a.wc_log;
        const int row = (int)(vrow & (Wc - 1));
        const bool valid = doc < C && row < a.c.len[doc < C ? doc : 0];
        const float* src = valid ? a.c.rows + ((int64_t)a.c.start[doc] + row) * kD + 8 * gs : nullptr;
        float* dst = As + R * kXStride + 8 * gs;
#pragma unroll 4
        for (int s = 0; s < kD / 32; ++s) {
            *reinterpret_cast<f32x4*>(dst + 32 * s) = valid ? ld4(src + 32 * s) : zero;
            *reinterpret_cast<f32x4*>(dst + 32 * s + 4) = valid ? ld4(src + 32 * s + 4) : zero;
        }
    }
    __syncthreads();
    const int64_t n_chunks = (Q * Wq + 15) / 16;
    for (int64_t qc = wave; qc < n_chunks; qc += 4) {
        const int64_t vq = qc * 16 + r, qdoc = vq >> a.wq_log;
        const int qrow = (int)(vq & (Wq - 1));
        const int qlen = qdoc < Q ? a.q.len[qdoc] : 0;
        const bool vb = qrow < qlen;
        const float* pb = a.q.rows + (vb ? ((int64_t)a.q.start[qdoc] + qrow) * kD : 0) + 8 * g;
        f32x4 acc0[4][4], acc1[4][4];
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int e = 0; e < 4; ++e) acc0[u][e] = acc1[u][e] = zero;
        f32x4 b0 = vb ? ld4(pb) : zero, b1 = vb ? ld4(pb + 4) : zero;
#pragma unroll 1
        for (int s0 = 0; s0 < kD / 32; s0 += 4) {
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                // the next block's query values are in flight while this block's 16 products issue
                const int s = s0 + u;
                const bool more = vb && s + 1 < kD / 32;
                const f32x4 n0 = more ? ld4(pb + 32 * (s + 1)) : zero, n1 = more ? ld4(pb + 32 * (s + 1) + 4) : zero;
                const float* la = As + r * kXStride + 32 * s + 8 * g;
                const f32x4 x0 = *reinterpret_cast<const f32x4*>(la), x1 = *reinterpret_cast<const f32x4*>(la + 4);
                const f32x4 y0 = *reinterpret_cast<const f32x4*>(la + 16 * kXStride), y1 = *reinterpret_cast<const f32x4*>(la + 16 * kXStride + 4);
                mfma8(x0, x1, b0, b1, acc0[u]);
                mfma8(y0, y1, b0, b1, acc1[u]);
                b0 = n0;
                b1 = n1;
            }
        }
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const f32x4 dot = t == 0 ? tile_dots(acc0) : tile_dots(acc1);
            bool valid[4];
            float m[4], S[4], T[4];
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const int64_t vrow = slot0 + 16 * t + 4 * g + v, cdoc = vrow >> a.wc_log;
                const int crow = (int)(vrow & (Wc - 1));
                valid[v] = vb && cdoc < C && crow < a.c.len[cdoc < C ? cdoc : 0];
                m[v] = valid[v] ? dot[v] : -INFINITY;
            }
            pair_block_allreduce(m, Wq, Wc, [](float x, float y) { return fmaxf(x, y); });
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const float y = dot[v] - m[v];
                S[v] = valid[v] ? shifted_exp(y) : 0.0f;
                T[v] = valid[v] ? S[v] * y : 0.0f;
            }
            pair_block_allreduce(S, Wq, Wc, [](float x, float y) { return x + y; });
            pair_block_allreduce(T, Wq, Wc, [](float x, float y) { return x + y; });
            const int vstep = Wc < 4 ? Wc : 4;
            const bool g_writes = Wc < 8 || (g & (Wc / 4 - 1)) == 0;
            if ((r & (Wq - 1)) == 0 && qdoc < Q && g_writes) {
#pragma unroll
                for (int v = 0; v < 4; ++v) {
                    if (v % vstep) continue;
                    const int64_t cdoc = (slot0 + 16 * t + 4 * g + v) >> a.wc_log;
                    if (cdoc >= C) continue;
                    const bool too_long = qlen > a.q.bound || a.c.len[cdoc] > a.c.bound;     // (the bound, not its row slots)
                    a.scores[qdoc * C + cdoc] = too_long ? __builtin_nanf("") : 2.0f * (m[v] + T[v] / S[v]);
                }
            }
        }
    }
}

int launch_pairs(const JsmArgs& a, int64_t P, hipStream_t s) {
    ASPIRE_REQUIRE((P + 3) / 4 < ((int64_t)1 << 31), ASPIRE_ERR_UNSUPPORTED, "too many pairs: %lld", (long long)P);
    hipLaunchKernelGGL(jointsm_pair_kernel, dim3((unsigned)((P + 3) / 4)), dim3(256), 0, s, a, P);
    ASPIRE_LAUNCH_OK();
    return ASPIRE_OK;
}

}  // namespace
}  // namespace aspire

using namespace aspire;

extern "C" int aspire_jointsm_scores_f32(const aspire_repset* q, const aspire_repset* c, int64_t D, int pairing, float* scores,
                                         float* pair_softmax, void* stream) {
    if (int rc = check_dot_sets(q, c, D, pairing, ASPIRE_SIM_DOT)) return rc;
    ASPIRE_REQUIRE(!pair_softmax || (q->ext > 0 && c->ext > 0), ASPIRE_ERR_INVALID_ARG,
                   "pair_softmax needs padded rep sets (ext > 0): its extents are [P, q.ext, c.ext]");
    if (q->n == 0 || c->n == 0) return ASPIRE_OK;
    ASPIRE_REQUIRE(scores, ASPIRE_ERR_INVALID_ARG, "scores is null");
    JsmArgs a{};
    a.q = to_dot(q);
    a.c = to_dot(c);
    a.scores = scores;
    a.pair_softmax = pair_softmax;
    hipStream_t s = (hipStream_t)stream;
    if (pairing == ASPIRE_PAIR_CROSS && a.q.bound <= 16 && a.c.bound <= 16 && !pair_softmax) {
        a.mode = kModeCross;
        a.wq_log = log2_slots(a.q.bound);
        a.wc_log = log2_slots(a.c.bound);
        const int64_t blocks = ((c->n << a.wc_log) + kXRows - 1) / kXRows;
        ASPIRE_REQUIRE(blocks < ((int64_t)1 << 31), ASPIRE_ERR_UNSUPPORTED, "too many candidates: %lld", (long long)c->n);
        hipLaunchKernelGGL(jointsm_cross_kernel, dim3((unsigned)blocks), dim3(256), 0, s, a);
        ASPIRE_LAUNCH_OK();
        return ASPIRE_OK;
    }
    a.mode = pairing == ASPIRE_PAIR_CROSS ? kModeCross : kModePaired;
    return launch_pairs(a, pairing == ASPIRE_PAIR_CROSS ? q->n * c->n : q->n, s);
}

extern "C" size_t aspire_jointsm_rank_batch_workspace_bytes(const aspire_repset* q, const aspire_repset* c, int64_t max_job, int64_t k) {
    if (!q || !c || q->n <= 0 || c->n <= 0 || k <= 0) return 0;
    return aspire_topk_workspace_bytes(q->n, max_job, k);
}

extern "C" int aspire_jointsm_rank_batch_f32(const aspire_repset* q, const aspire_repset* c, int64_t D, const int32_t* job_off,
                                             int64_t max_job, float* scores, int64_t k, const int32_t* job_base,
                                             float* top_scores, int64_t* top_idx, uint64_t* keys, void* workspace,
                                             size_t workspace_bytes, void* stream) {
    if (int rc = check_dot_sets(q, c, D, ASPIRE_PAIR_CROSS, ASPIRE_SIM_DOT)) return rc;
    const int64_t J = q->n, C = c->n;
    BatchRank rank{J, max_job, k, top_scores, top_idx, keys, job_off, job_base, stream};
    bool go_on;
    if (int rc = batch_preamble(q, c, scores, rank, go_on); !go_on) return rc;
    const size_t need = aspire_jointsm_rank_batch_workspace_bytes(q, c, max_job, k);
    ASPIRE_REQUIRE(workspace_bytes >= need && (need == 0 || workspace), ASPIRE_ERR_INVALID_ARG,
                   "workspace too small: %zu bytes given, aspire_jointsm_rank_batch_workspace_bytes says %zu", workspace_bytes, need);
    ASPIRE_REQUIRE(((uintptr_t)workspace & 15) == 0, ASPIRE_ERR_INVALID_ARG, "workspace must be 16-byte aligned");
    rank.scratch_at(workspace);
    JsmArgs a{};
    a.q = to_dot(q);
    a.c = to_dot(c);
    a.scores = scores;
    a.mode = kModeMapped;
    a.job_off = job_off;
    a.J = (int32_t)J;
    if (int rc = launch_pairs(a, C, (hipStream_t)stream)) return rc;
    return rank.rank(scores);
}
