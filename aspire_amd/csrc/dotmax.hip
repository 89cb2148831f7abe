// Max over sentence pairs of a dot-product similarity: the cosentbert / ictsentbert score (include/aspire_hip.h, A13).
//
//   score(q, c) = max over valid (i < q_len, j < c_len) of sim(q_i, c_j)
//   COSINE  sklearn.metrics.pairwise.cosine_similarity on float32 rows (TrainedSentModel.get_similarity,
//           src/evaluation/utils/models.py:602-604): every row divided by n = sqrt(fp32 sum of squares), an n below
//           10 * FLT_EPSILON replaced by 1 (sklearn's _handle_zeros_in_scale), then the dot.  A row whose n is inf
//           divides to zeros: it scores 0 against everything, whatever the raw dot.
//   DOT     the raw dot (np.matmul; pp_gen_nearest.py rank_pool_sent, score_aggregation 'dotlse').
//
// Both kernels stand in pair_fwd.h's frame (the wave's pair and its poison rule, the tile walk, the staged row slots, the writers) and
// keep their own k loops and epilogues.  Both run the dot products on v_mfma_f32_16x16x4_f32 (exact fp32, a bitwise fmaf chain per accumulator) with four
// independent accumulators over k per 16 x 16 tile, form the squared row norms with fmaf from the same registers the matrix
// products read, and do the validity mask, the normalisation and the max in the epilogue: the [rows_q, rows_c] similarity block
// is never written.  A lane holds A[row l & 15][k] and B[k][col l & 15] for k = 32 s + 8 (l >> 4) + e: the k order inside a
// block of 32 is permuted identically for both operands, so the sums are the same dot products.
//   dotmax_cross_kernel  CROSS with documents of <= 16 rows (config 3's shape: a few dozen queries against a resident store).
//                        A workgroup holds 32 candidate row slots (documents padded to a power of two W_c <= 16, so 32 / W_c
//                        documents) in LDS, read from HBM once, and its four waves stream the query rows (L2-resident) in
//                        chunks of 16 slots.
//   dotmax_pair_kernel   one wave per (query, candidate) pair, 16 x 16 tiles over documents of up to 128 rows: PAIRED, the
//                        jobs of aspire_dotmax_rank_batch_f32 (candidate p against its job's query) and CROSS with longer
//                        documents.
#include <float.h>
#include <math.h>

#include "common.h"
#include "batch_host.h"
#include "pair_fwd.h"

namespace aspire {
namespace {

struct DotArgs : PairArgs {
    int sim;
};

// sklearn's row norm from the fp32 sum of squares: its square root, near-zero -> 1
__device__ __forceinline__ float sklearn_norm(float ss) {
    const float n = sqrtf(ss);
    return n < 10.0f * FLT_EPSILON ? 1.0f : n;
}

__device__ __forceinline__ float finish(float dot, float nq, float nc, int sim) {
    if (sim == ASPIRE_SIM_DOT) return dot;
    if (isinf(nq) || isinf(nc)) return 0.0f;      // x / inf = 0 row: no inf / inf
    return dot / nq / nc;
}

// ---- one wave per pair (pair_fwd.h) --------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) dotmax_pair_kernel(DotArgs a, int64_t P) {
    const int64_t p = wave_pair();
    if (p >= P) return;
    const PairWave w = pair_wave(a.q, a.c, a.mode, a.job_off, a.J, p);
    if (w.poison) return poison_score(a.scores, p, w.lane);
    float best = -INFINITY;
    const float *qbase = w.qdoc + 8 * w.g, *cbase = w.cdoc + 8 * w.g;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    for (int c0 = 0; c0 < w.cl; c0 += 16) {
        const bool va = tile_row_valid(w.r, c0, w.cl);
        const float* pa = tile_row(w.r, cbase, c0, w.cl);
        for (int q0 = 0; q0 < w.ql; q0 += 16) {
            const bool vb = tile_row_valid(w.r, q0, w.ql);
            const float* pb = tile_row(w.r, qbase, q0, w.ql);
            f32x4 acc[4] = {zero, zero, zero, zero};
            float ssa = 0.f, ssb = 0.f;
            for (int s = 0; s < kD / 32; ++s) {
                const f32x4 a0 = va ? ld4(pa + 32 * s) : zero, a1 = va ? ld4(pa + 32 * s + 4) : zero;
                const f32x4 b0 = vb ? ld4(pb + 32 * s) : zero, b1 = vb ? ld4(pb + 32 * s + 4) : zero;
                ssa = sumsq8(ssa, a0, a1);
                ssb = sumsq8(ssb, b0, b1);
                mfma8(a0, a1, b0, b1, acc);
            }
            const float nb = sklearn_norm(rowgroup_sum(ssb));
            const float na_own = sklearn_norm(rowgroup_sum(ssa));
            const f32x4 dot = (acc[0] + acc[1]) + (acc[2] + acc[3]);
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const float na = __shfl(na_own, 4 * w.g + v);
                const float x = finish(dot[v], nb, na, a.sim);
                if (entry_valid(w, c0, v, vb)) best = fmaxf(best, x);
            }
        }
    }
    best = wave_max(best);
    if (w.lane == 0) a.scores[p] = best;
}

// ---- CROSS, documents of <= 16 rows: 32 candidate row slots per workgroup in LDS (pair_fwd.h) ----------------------------
__global__ void __launch_bounds__(256) dotmax_cross_kernel(DotArgs a) {
    __shared__ __attribute__((aligned(16))) float As[kXRows * kXStride];
    __shared__ float nrm_c[kXRows];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, r = lane & 15;
    const int Wc = 1 << a.wc_log, Wq = 1 << a.wq_log;
    const int64_t slot0 = (int64_t)blockIdx.x * kXRows;
    stage_slots<true>(a.c, a.wc_log, slot0, As, nrm_c);
    __syncthreads();
    const int64_t n_chunks = (a.q.n * Wq + 15) / 16;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    for (int64_t qc = wave; qc < n_chunks; qc += 4) {
        const QueryChunk k = query_chunk(a.q, a.wq_log, qc, g, r);
        const bool vb = k.vb;
        const float* pb = k.pb;
        f32x4 acc0[4] = {zero, zero, zero, zero}, acc1[4] = {zero, zero, zero, zero};
        float ssb = 0.f;
        f32x4 b0 = vb ? ld4(pb) : zero, b1 = vb ? ld4(pb + 4) : zero;
#pragma unroll 2
        for (int s = 0; s < kD / 32; ++s) {
            // the next block's query values are in flight while this block's 16 products issue
            const bool more = vb && s + 1 < kD / 32;
            const f32x4 n0 = more ? ld4(pb + 32 * (s + 1)) : zero, n1 = more ? ld4(pb + 32 * (s + 1) + 4) : zero;
            const float* la = As + r * kXStride + 32 * s + 8 * g;
            const f32x4 x0 = *reinterpret_cast<const f32x4*>(la), x1 = *reinterpret_cast<const f32x4*>(la + 4);
            const f32x4 y0 = *reinterpret_cast<const f32x4*>(la + 16 * kXStride), y1 = *reinterpret_cast<const f32x4*>(la + 16 * kXStride + 4);
            ssb = sumsq8(ssb, b0, b1);
            mfma8(x0, x1, b0, b1, acc0);
            mfma8(y0, y1, b0, b1, acc1);
            b0 = n0;
            b1 = n1;
        }
        const float nb = sklearn_norm(rowgroup_sum(ssb));
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const f32x4 dot = t == 0 ? (acc0[0] + acc0[1]) + (acc0[2] + acc0[3]) : (acc1[0] + acc1[1]) + (acc1[2] + acc1[3]);
            float m[4];
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const int R = 16 * t + 4 * g + v;
                const bool va = slot_of(a.c, a.wc_log, slot0 + R).valid;
                const float x = finish(dot[v], nb, sklearn_norm(nrm_c[R]), a.sim);
                m[v] = va && vb ? x : -INFINITY;
                // the query document's rows sit on Wq neighbouring lanes
                for (int sh = 1; sh < Wq; sh <<= 1) m[v] = fmaxf(m[v], __shfl_xor(m[v], sh));
            }
            // the candidate document's rows: Wc neighbouring rows = registers v, then lane groups g -- a one-way max towards the
            // writers (pair_block_allreduce would spend moves on the lanes that do not write; fmaxf is exact either way)
            if (Wc >= 2) {
                m[0] = fmaxf(m[0], m[1]);
                m[2] = fmaxf(m[2], m[3]);
            }
            if (Wc >= 4) m[0] = fmaxf(m[0], m[2]);
            if (Wc >= 8) m[0] = fmaxf(m[0], __shfl_xor(m[0], 16));
            if (Wc >= 16) m[0] = fmaxf(m[0], __shfl_xor(m[0], 32));
            write_pair_scores(a, slot0, t, g, r, k, [=](int v) { return m[v]; });
        }
    }
}

}  // namespace
}  // namespace aspire

using namespace aspire;

extern "C" int aspire_dotmax_scores_f32(const aspire_repset* q, const aspire_repset* c, int64_t D, int pairing, int sim,
                                        float* scores, void* stream) {
    if (int rc = check_dot_sets(q, c, D, pairing, sim)) return rc;
    if (q->n == 0 || c->n == 0) return ASPIRE_OK;
    ASPIRE_REQUIRE(scores, ASPIRE_ERR_INVALID_ARG, "scores is null");
    DotArgs a{pair_args(q, c, pairing, scores), sim};
    if (pairing == ASPIRE_PAIR_CROSS && cross_form(a)) return launch_cross_slots(dotmax_cross_kernel, a, (hipStream_t)stream);
    return launch_pair_waves(dotmax_pair_kernel, a, pairing == ASPIRE_PAIR_CROSS ? q->n * c->n : q->n, (hipStream_t)stream);
}

extern "C" size_t aspire_dotmax_rank_batch_workspace_bytes(const aspire_repset* q, const aspire_repset* c, int64_t max_job, int64_t k) {
    return rank_scratch_only_bytes(q, c, max_job, k);
}

extern "C" int aspire_dotmax_rank_batch_f32(const aspire_repset* q, const aspire_repset* c, int64_t D, const int32_t* job_off,
                                            int64_t max_job, int sim, float* scores, int64_t k, const int32_t* job_base,
                                            float* top_scores, int64_t* top_idx, uint64_t* keys, void* workspace,
                                            size_t workspace_bytes, void* stream) {
    if (int rc = check_dot_sets(q, c, D, ASPIRE_PAIR_CROSS, sim)) return rc;
    const int64_t J = q->n, C = c->n;
    BatchRank rank{J, max_job, k, top_scores, top_idx, keys, job_off, job_base, stream};
    bool go_on;
    if (int rc = batch_preamble(q, c, scores, rank, go_on); !go_on) return rc;
    if (int rc = place_scratch(rank, workspace, workspace_bytes, rank_scratch_only_bytes(q, c, max_job, k), 0,
                               "aspire_dotmax_rank_batch_workspace_bytes")) return rc;
    const DotArgs a{mapped_pair_args(q, c, job_off, scores), sim};
    if (int rc = launch_pair_waves(dotmax_pair_kernel, a, C, (hipStream_t)stream)) return rc;
    return rank.rank(scores);
}
