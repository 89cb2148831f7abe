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
// S <- f S, T <- f (T + (m - m') S) (pair_fwd.h: CentredSoftmax).
//   jointsm_pair_kernel   one wave per (query, candidate) pair, 16 x 16 tiles over documents of up to 128 rows, m wave-uniform
//                         (one wave_max per tile), S and T per lane until the end: PAIRED, the jobs of
//                         aspire_jointsm_rank_batch_f32, CROSS with longer documents, and every call that wants pair_softmax
//                         (pass 1 leaves d_ij in the output block, pass 2 -- every lane over its own entries -- turns them
//                         into p_ij once m and S are final, then the pad entries are zeroed).
//   jointsm_cross_kernel  CROSS with documents of <= 16 rows: pair_fwd.h's cross layout (32 candidate row slots per workgroup in
//                         LDS, the query rows streamed in chunks of 16 slots); max, S and T are segmented all-reductions over the
//                         W_q lanes x W_c rows of a document pair.
// The two kernels sum S and T in different orders: a pair's score agrees between them to rounding, not
// in every bit.
#include <math.h>

#include "common.h"
#include "batch_host.h"
#include "pair_fwd.h"

namespace aspire {
namespace {

struct JsmArgs : PairArgs {
    float* pair_softmax;        // pair kernel, padded sets: [P, q.bound, c.bound], or null
};

// exp((d - m) / sqrt(encoding_dim)) for d <= m: torch.div(pair_sims, math.sqrt(encoding_dim)) behind the max shift
__device__ __forceinline__ float shifted_exp(float y) { return expf(y / sqrtf((float)kD)); }

// ---- one wave per pair (pair_fwd.h) --------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) jointsm_pair_kernel(JsmArgs a, int64_t P) {
    const int64_t p = wave_pair();
    if (p >= P) return;
    const PairWave w = pair_wave(a.q, a.c, a.mode, a.job_off, a.J, p);
    const int lane = w.lane, g = w.g, r = w.r, ql = w.ql, cl = w.cl;
    const int qext = a.q.bound, cext = a.c.bound;
    float* soft = a.pair_softmax ? a.pair_softmax + p * qext * cext : nullptr;
    if (w.poison) {
        poison_score(a.scores, p, lane);
        if (soft)
            for (int e = lane; e < qext * cext; e += 64) soft[e] = __builtin_nanf("");
        return;
    }
    const float *qbase = w.qdoc + 8 * g, *cbase = w.cdoc + 8 * g;
    CentredSoftmax sm;
    const auto ex = [](float y) { return shifted_exp(y); };
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    for (int c0 = 0; c0 < cl; c0 += 16) {
        const bool va = tile_row_valid(r, c0, cl);
        const float* pa = tile_row(r, cbase, c0, cl);
        for (int q0 = 0; q0 < ql; q0 += 16) {
            const bool vb = tile_row_valid(r, q0, ql);
            const float* pb = tile_row(r, qbase, q0, ql);
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
            const f32x4 dot = tile_dots(acc);
            float tile_max = -INFINITY;
#pragma unroll
            for (int v = 0; v < 4; ++v)
                if (entry_valid(w, c0, v, vb)) tile_max = fmaxf(tile_max, dot[v]);
            sm.raise(wave_max(tile_max), ex);
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                if (entry_valid(w, c0, v, vb)) {
                    sm.add(dot[v], ex);
                    if (soft) soft[(q0 + r) * cext + c0 + 4 * g + v] = dot[v];
                }
            }
        }
    }
    const float m = sm.m, S = wave_sum(sm.S), T = wave_sum(sm.T);
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

// ---- CROSS, documents of <= 16 rows: 32 candidate row slots per workgroup in LDS (pair_fwd.h) ----------------------------
__global__ void __launch_bounds__(256) jointsm_cross_kernel(JsmArgs a) {
    __shared__ __attribute__((aligned(16))) float As[kXRows * kXStride];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, r = lane & 15;
    const int Wc = 1 << a.wc_log, Wq = 1 << a.wq_log;
    const int64_t slot0 = (int64_t)blockIdx.x * kXRows;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    stage_slots<false>(a.c, a.wc_log, slot0, As, nullptr);
    __syncthreads();
    const int64_t n_chunks = (a.q.n * Wq + 15) / 16;
    for (int64_t qc = wave; qc < n_chunks; qc += 4) {
        const QueryChunk k = query_chunk(a.q, a.wq_log, qc, g, r);
        f32x4 acc0[4][4], acc1[4][4];
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int e = 0; e < 4; ++e) acc0[u][e] = acc1[u][e] = zero;
        f32x4 b0 = k.vb ? ld4(k.pb) : zero, b1 = k.vb ? ld4(k.pb + 4) : zero;
#pragma unroll 1
        for (int s0 = 0; s0 < kD / 32; s0 += 4) {
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                // the next block's query values are in flight while this block's 16 products issue
                const int s = s0 + u;
                const bool more = k.vb && s + 1 < kD / 32;
                const f32x4 n0 = more ? ld4(k.pb + 32 * (s + 1)) : zero, n1 = more ? ld4(k.pb + 32 * (s + 1) + 4) : zero;
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
                valid[v] = k.vb && slot_of(a.c, a.wc_log, slot0 + 16 * t + 4 * g + v).valid;
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
            write_pair_scores(a, slot0, t, g, r, k, [=](int v) { return 2.0f * (m[v] + T[v] / S[v]); });
        }
    }
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
    JsmArgs a{pair_args(q, c, pairing, scores), pair_softmax};
    if (pairing == ASPIRE_PAIR_CROSS && cross_form(a) && !pair_softmax) return launch_cross_slots(jointsm_cross_kernel, a, (hipStream_t)stream);
    return launch_pair_waves(jointsm_pair_kernel, a, pairing == ASPIRE_PAIR_CROSS ? q->n * c->n : q->n, (hipStream_t)stream);
}

extern "C" size_t aspire_jointsm_rank_batch_workspace_bytes(const aspire_repset* q, const aspire_repset* c, int64_t max_job, int64_t k) {
    return rank_scratch_only_bytes(q, c, max_job, k);
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
    if (int rc = place_scratch(rank, workspace, workspace_bytes, rank_scratch_only_bytes(q, c, max_job, k), 0,
                               "aspire_jointsm_rank_batch_workspace_bytes")) return rc;
    const JsmArgs a{mapped_pair_args(q, c, job_off, scores), nullptr};
    if (int rc = launch_pair_waves(jointsm_pair_kernel, a, C, (hipStream_t)stream)) return rc;
    return rank.rank(scores);
}
