// Max over sentence pairs of a dot-product similarity: the cosentbert / ictsentbert score (include/aspire_hip.h, A13).
//
//   score(q, c) = max over valid (i < q_len, j < c_len) of sim(q_i, c_j)
//   COSINE  sklearn.metrics.pairwise.cosine_similarity on float32 rows (TrainedSentModel.get_similarity,
//           src/evaluation/utils/models.py:602-604): every row divided by n = sqrt(fp32 sum of squares), an n below
//           10 * FLT_EPSILON replaced by 1 (sklearn's _handle_zeros_in_scale), then the dot.  A row whose n is inf
//           divides to zeros: it scores 0 against everything, whatever the raw dot.
//   DOT     the raw dot (np.matmul; pp_gen_nearest.py rank_pool_sent, score_aggregation 'dotlse').
//
// Both kernels run the dot products on v_mfma_f32_16x16x4_f32 (exact fp32, a bitwise fmaf chain per accumulator) with four
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
#include "dot_tiles.h"

namespace aspire {
namespace {

struct DotArgs {
    DotSet q, c;
    int sim;
    int mode;
    const int32_t* job_off;     // kModeMapped: [J + 1]
    int32_t J;
    int32_t wq_log, wc_log;     // cross kernel: log2 of the row slots per document
    float* scores;
};

// sklearn's row norm: sqrt of the fp32 sum of squares, near-zero -> 1
__device__ __forceinline__ float row_norm(float ss) {
    const float n = sqrtf(ss);
    return n < 10.0f * FLT_EPSILON ? 1.0f : n;
}

__device__ __forceinline__ float finish(float dot, float nq, float nc, int sim) {
    if (sim == ASPIRE_SIM_DOT) return dot;
    if (isinf(nq) || isinf(nc)) return 0.0f;      // x / inf = 0 row: no inf / inf
    return dot / nq / nc;
}

__device__ __forceinline__ float sumsq8(float ss, const f32x4& x0, const f32x4& x1) {
    ss = fmaf(x0.x, x0.x, ss);
    ss = fmaf(x0.y, x0.y, ss);
    ss = fmaf(x0.z, x0.z, ss);
    ss = fmaf(x0.w, x0.w, ss);
    ss = fmaf(x1.x, x1.x, ss);
    ss = fmaf(x1.y, x1.y, ss);
    ss = fmaf(x1.z, x1.z, ss);
    return fmaf(x1.w, x1.w, ss);
}

// the four lanes that share l & 15 hold the partial sums of one row
__device__ __forceinline__ float rowgroup_sum(float v) {
    v += lane_xor<16>(v);
    return v + lane_xor<32>(v);
}

// ---- one wave per pair --------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) dotmax_pair_kernel(DotArgs a, int64_t P) {
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
    if (ql > a.q.bound || cl > a.c.bound) {
        if (lane == 0) a.scores[p] = __builtin_nanf("");
        return;
    }
    const float* qbase = a.q.rows + (int64_t)a.q.start[qi] * kD + 8 * g;
    const float* cbase = a.c.rows + (int64_t)a.c.start[ci] * kD + 8 * g;
    float best = -INFINITY;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    for (int c0 = 0; c0 < cl; c0 += 16) {
        const bool va = c0 + r < cl;
        const float* pa = cbase + (int64_t)(va ? c0 + r : 0) * kD;
        for (int q0 = 0; q0 < ql; q0 += 16) {
            const bool vb = q0 + r < ql;
            const float* pb = qbase + (int64_t)(vb ? q0 + r : 0) * kD;
            f32x4 acc[4] = {zero, zero, zero, zero};
            float ssa = 0.f, ssb = 0.f;
            for (int s = 0; s < kD / 32; ++s) {
                const f32x4 a0 = va ? ld4(pa + 32 * s) : zero, a1 = va ? ld4(pa + 32 * s + 4) : zero;
                const f32x4 b0 = vb ? ld4(pb + 32 * s) : zero, b1 = vb ? ld4(pb + 32 * s + 4) : zero;
                ssa = sumsq8(ssa, a0, a1);
                ssb = sumsq8(ssb, b0, b1);
                mfma8(a0, a1, b0, b1, acc);
            }
            // C[row 4 g + v][col r]: candidate row c0 + 4 g + v, query row q0 + r
            const float nb = row_norm(rowgroup_sum(ssb));
            const float na_own = row_norm(rowgroup_sum(ssa));
            const f32x4 dot = (acc[0] + acc[1]) + (acc[2] + acc[3]);
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const float na = __shfl(na_own, 4 * g + v);
                const float x = finish(dot[v], nb, na, a.sim);
                if (c0 + 4 * g + v < cl && vb) best = fmaxf(best, x);
            }
        }
    }
    best = wave_max(best);
    if (lane == 0) a.scores[p] = best;
}

// ---- CROSS, documents of <= 16 rows: 32 candidate row slots per workgroup in LDS --------------------------------------
__global__ void __launch_bounds__(256) dotmax_cross_kernel(DotArgs a) {
    __shared__ __attribute__((aligned(16))) float As[kXRows * kXStride];
    __shared__ float nrm_c[kXRows];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, r = lane & 15;
    const int Wc = 1 << a.wc_log, Wq = 1 << a.wq_log;
    const int64_t C = a.c.n, Q = a.q.n;
    const int64_t slot0 = (int64_t)blockIdx.x * kXRows;
    // stage: four threads per row slot (waves 0 and 1), thread g reads k = 32 s + 8 g .. + 7 -- the k values lane group g of
    // dotmax_pair_kernel reads, summed in the same order, so the two kernels give the same bits for a pair
    if (tid < 4 * kXRows) {
        const int R = tid >> 2, gs = tid & 3;
        const int64_t vrow = slot0 + R, doc = vrow >> a.wc_log;
        const int row = (int)(vrow & (Wc - 1));
        const bool valid = doc < C && row < a.c.len[doc < C ? doc : 0];
        const float* src = valid ? a.c.rows + ((int64_t)a.c.start[doc] + row) * kD + 8 * gs : nullptr;
        float* dst = As + R * kXStride + 8 * gs;
        const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
        float ss = 0.f;
#pragma unroll 4
        for (int s = 0; s < kD / 32; ++s) {
            const f32x4 x0 = valid ? ld4(src + 32 * s) : zero, x1 = valid ? ld4(src + 32 * s + 4) : zero;
            ss = sumsq8(ss, x0, x1);
            *reinterpret_cast<f32x4*>(dst + 32 * s) = x0;
            *reinterpret_cast<f32x4*>(dst + 32 * s + 4) = x1;
        }
        ss += lane_xor<1>(ss);             // (g0 + g1) + (g2 + g3), as rowgroup_sum
        ss += lane_xor<2>(ss);
        if (gs == 0) nrm_c[R] = ss;
    }
    __syncthreads();
    const int64_t n_chunks = (Q * Wq + 15) / 16;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    for (int64_t qc = wave; qc < n_chunks; qc += 4) {
        const int64_t vq = qc * 16 + r, qdoc = vq >> a.wq_log;
        const int qrow = (int)(vq & (Wq - 1));
        const int qlen = qdoc < Q ? a.q.len[qdoc] : 0;
        const bool vb = qrow < qlen;
        const float* pb = a.q.rows + (vb ? ((int64_t)a.q.start[qdoc] + qrow) * kD : 0) + 8 * g;
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
        const float nb = row_norm(rowgroup_sum(ssb));
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const f32x4 dot = t == 0 ? (acc0[0] + acc0[1]) + (acc0[2] + acc0[3]) : (acc1[0] + acc1[1]) + (acc1[2] + acc1[3]);
            float m[4];
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const int R = 16 * t + 4 * g + v;
                const int64_t vrow = slot0 + R, cdoc = vrow >> a.wc_log;
                const int crow = (int)(vrow & (Wc - 1));
                const bool va = cdoc < C && crow < a.c.len[cdoc < C ? cdoc : 0];
                const float x = finish(dot[v], nb, row_norm(nrm_c[R]), a.sim);
                m[v] = va && vb ? x : -INFINITY;
                // the query document's rows sit on Wq neighbouring lanes
                for (int sh = 1; sh < Wq; sh <<= 1) m[v] = fmaxf(m[v], __shfl_xor(m[v], sh));
            }
            // the candidate document's rows: Wc neighbouring rows = registers v, then lane groups g
            if (Wc >= 2) {
                m[0] = fmaxf(m[0], m[1]);
                m[2] = fmaxf(m[2], m[3]);
            }
            if (Wc >= 4) m[0] = fmaxf(m[0], m[2]);
            if (Wc >= 8) m[0] = fmaxf(m[0], __shfl_xor(m[0], 16));
            if (Wc >= 16) m[0] = fmaxf(m[0], __shfl_xor(m[0], 32));
            const int vstep = Wc < 4 ? Wc : 4;
            const bool g_writes = Wc < 8 || (g & (Wc / 4 - 1)) == 0;
            if ((r & (Wq - 1)) == 0 && qdoc < Q && g_writes) {
#pragma unroll
                for (int v = 0; v < 4; ++v) {
                    if (v % vstep) continue;
                    const int64_t cdoc = (slot0 + 16 * t + 4 * g + v) >> a.wc_log;
                    if (cdoc >= C) continue;
                    const bool too_long = qlen > a.q.bound || a.c.len[cdoc] > a.c.bound;     // (the bound, not its row slots)
                    a.scores[qdoc * C + cdoc] = too_long ? __builtin_nanf("") : m[v];
                }
            }
        }
    }
}

int launch_pairs(const DotArgs& a, int64_t P, hipStream_t s) {
    ASPIRE_REQUIRE((P + 3) / 4 < ((int64_t)1 << 31), ASPIRE_ERR_UNSUPPORTED, "too many pairs: %lld", (long long)P);
    hipLaunchKernelGGL(dotmax_pair_kernel, dim3((unsigned)((P + 3) / 4)), dim3(256), 0, s, a, P);
    ASPIRE_LAUNCH_OK();
    return ASPIRE_OK;
}

}  // namespace
}  // namespace aspire

using namespace aspire;

extern "C" int aspire_dotmax_scores_f32(const aspire_repset* q, const aspire_repset* c, int64_t D, int pairing, int sim,
                                        float* scores, void* stream) {
    if (int rc = check_dot_sets(q, c, D, pairing, sim)) return rc;
    if (q->n == 0 || c->n == 0) return ASPIRE_OK;
    ASPIRE_REQUIRE(scores, ASPIRE_ERR_INVALID_ARG, "scores is null");
    DotArgs a{};
    a.q = to_dot(q);
    a.c = to_dot(c);
    a.sim = sim;
    a.scores = scores;
    hipStream_t s = (hipStream_t)stream;
    if (pairing == ASPIRE_PAIR_CROSS && a.q.bound <= 16 && a.c.bound <= 16) {
        a.mode = kModeCross;
        a.wq_log = log2_slots(a.q.bound);
        a.wc_log = log2_slots(a.c.bound);
        const int64_t blocks = ((c->n << a.wc_log) + kXRows - 1) / kXRows;
        ASPIRE_REQUIRE(blocks < ((int64_t)1 << 31), ASPIRE_ERR_UNSUPPORTED, "too many candidates: %lld", (long long)c->n);
        hipLaunchKernelGGL(dotmax_cross_kernel, dim3((unsigned)blocks), dim3(256), 0, s, a);
        ASPIRE_LAUNCH_OK();
        return ASPIRE_OK;
    }
    a.mode = pairing == ASPIRE_PAIR_CROSS ? kModeCross : kModePaired;
    return launch_pairs(a, pairing == ASPIRE_PAIR_CROSS ? q->n * c->n : q->n, s);
}

extern "C" size_t aspire_dotmax_rank_batch_workspace_bytes(const aspire_repset* q, const aspire_repset* c, int64_t max_job, int64_t k) {
    if (!q || !c || q->n <= 0 || c->n <= 0 || k <= 0) return 0;
    return aspire_topk_workspace_bytes(q->n, max_job, k);
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
    const size_t need = aspire_dotmax_rank_batch_workspace_bytes(q, c, max_job, k);
    ASPIRE_REQUIRE(workspace_bytes >= need && (need == 0 || workspace), ASPIRE_ERR_INVALID_ARG,
                   "workspace too small: %zu bytes given, aspire_dotmax_rank_batch_workspace_bytes says %zu", workspace_bytes, need);
    ASPIRE_REQUIRE(((uintptr_t)workspace & 15) == 0, ASPIRE_ERR_INVALID_ARG, "workspace must be 16-byte aligned");
    rank.scratch_at(workspace);
    DotArgs a{};
    a.q = to_dot(q);
    a.c = to_dot(c);
    a.sim = sim;
    a.scores = scores;
    a.mode = kModeMapped;
    a.job_off = job_off;
    a.J = (int32_t)J;
    if (int rc = launch_pairs(a, C, (hipStream_t)stream)) return rc;
    return rank.rank(scores);
}
