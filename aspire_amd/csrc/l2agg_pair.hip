// The sibling aggregations of the negated L2 block over batched jobs: 'l2top2' and 'l2attention' (include/aspire_hip.h,
// aspire_l2agg_rank_batch_f32; allpair_masked_dist_l2topk, pair_distances.py:295-345, and AllPairMaskedAttention, :95-135).
//
//   d_ij  = sqrt(max(|q_i|^2 + |c_j|^2 - 2 <q_i, c_j>, 0))        over the valid block (i < q_len, j < c_len), s_ij = -d_ij
//   TOP2       score = the sum of the two largest s_ij (by entries: two equal distances both count, as torch.topk(k = 2) counts
//              them); a 1 x 1 block takes -10e8 as the missing one (the header's contract for rep sets without padded extents)
//   ATTENTION  score = sum_ij p_ij s_ij,  p = soft-max of s_ij / temp over the valid block
//
// One kernel, l2agg_pair_kernel<AGG>: one wave per (candidate, its job's query) pair, four pairs per workgroup, 16 x 16 tiles over
// documents of 1 .. 128 rows -- pair_fwd.h's one-wave-per-pair frame (kModeMapped) with its own tile epilogue.  One form for every call size:
// a pair's bits depend on its two documents only.
//
// Dot products: dot_tiles.h (exact fp32 on v_mfma_f32_16x16x4_f32) over SIXTEEN accumulators per tile, as jointsm.hip.  What counts
// here is d^2 = |q|^2 + |c|^2 - 2 q.c, whose three terms are each far larger than their difference once rows share a common
// component: at the cancel rule's own threshold (below) d^2 = 1e-4 (|q|^2 + |c|^2)^2, so a relative error e of the 2 q.c term
// reaches the distance as e (|q|^2 + |c|^2) / 2 d = 50 e (unit-free: it does not depend on the rows' scale).  jointsm.hip's header
// measured e = 2.7e-7 for four chains of 192 (1.4e-5 in d) and 6e-8 for sixteen of 48 (3e-6); with the two norms' error beside it
// four chains would spend a quarter of the 1e-4 parity bar on the kernel's own rounding, sixteen a twentieth.  The registers are
// there (two waves per SIMD).
// Row norms: from the SAME loaded operands -- no pre-pass and no second read.  A lane squares the 8 k values per block it holds of
// its A row (candidate row c0 + r) and of its B row (query row q0 + r) into four chains each (the x / y / z / w of an f32x4: 48 fmaf
// per chain, the dots' chain length), the four lane groups' partial sums are added across lanes 16 and 32 apart (the same bits in
// all four), and the candidate norm of accumulator row 4 g + v is read from lane 4 g + v.  A row's norm is recomputed in every tile
// it takes part in -- 8 VALU fmaf per 8 MFMAs, hidden under the matrix pipe -- from its own values in one fixed order: the same bits
// in every tile and every pair.
// SHARED SENTENCES (include/aspire_hip.h): an entry with d^2 < 1e-4 (|q|^2 + |c|^2)^2 is redone by its lane from the exact sum of
// squared differences (exact_d2: the arithmetic of generic.hip's cancelling entries and gram.hip's direct_d2), so a shared sentence
// scores -d ~ 0, not -sqrt(rounding noise).
// ATTENTION keeps the soft-max shifted by the running maximum m of s (wave-uniform: one wave_max per tile) and sums, beside
// S = sum e_ij with e_ij = expf((s_ij - m) / temp), the CENTRED T = sum e_ij (s_ij - m): score = m + T / S.  Scores are about -40
// and their spread a few units: T / S is a small correction to m, so the rounding of the two long sums reaches the score scaled
// down by that ratio.  A new maximum m' rescales with f = expf((m - m') / temp): S <- f S, T <- f (T + (m - m') S) (pair_fwd.h: CentredSoftmax).
// S and T stay per lane until the end, then wave_sum in its fixed order.  TOP2 keeps (first, second) per lane and merges them
// across the wave by entries; max / min only, so the order of the merge does not reach the bits.
#include <math.h>

#include "common.h"
#include "batch_host.h"
#include "pair_fwd.h"
#include "exact_d2.h"

namespace aspire {
namespace {

struct L2aggArgs : PairArgs {
    float temp;                 // ATTENTION
};

// sum_d (x_d - y_d)^2 over the 768 coordinates (rare path: a candidate row that (nearly) equals a query row)
__device__ __noinline__ float exact_d2(const float* __restrict__ x, const float* __restrict__ y) {
    float s0 = 0.f, s1 = 0.f;
#pragma unroll 1           // exact_d2.h's form C, rolled: lane_d2 leaves the unrolling to the compiler, and this function's registers count in the kernel's
    for (int k = 0; k < kD; k += 8) d2_step2(ld4(x + k), ld4(y + k), ld4(x + k + 4), ld4(y + k + 4), s0, s1);
    return s0 + s1;
}

// |row|^2 of the lane's operand row from the four lane groups' chains: the same bits in the four lanes that share lane & 15
__device__ __forceinline__ float row_sumsq(const f32x4& n) { return rowgroup_sum((n.x + n.y) + (n.z + n.w)); }

// (first, second) of the union of two (first, second) pairs, by entries
__device__ __forceinline__ void top2_merge(float& t1, float& t2, float o1, float o2) {
    t2 = fmaxf(fminf(t1, o1), fmaxf(t2, o2));
    t1 = fmaxf(t1, o1);
}

template <int M>
__device__ __forceinline__ void top2_fold(float& t1, float& t2) {
    const float o1 = lane_xor<M>(t1), o2 = lane_xor<M>(t2);
    top2_merge(t1, t2, o1, o2);
}

template <int AGG>
__global__ void __launch_bounds__(256) l2agg_pair_kernel(L2aggArgs a, int64_t P) {
    static_assert(AGG == ASPIRE_AGG_TOP2 || AGG == ASPIRE_AGG_ATTENTION, "the batched siblings; max-sim has its own entry");
    const int64_t p = wave_pair();
    if (p >= P) return;
    const PairWave w = pair_wave(a.q, a.c, kModeMapped, a.job_off, a.J, p);
    const int lane = w.lane, g = w.g, r = w.r, ql = w.ql, cl = w.cl;
    if (w.poison) return poison_score(a.scores, p, lane);
    const float *qdoc = w.qdoc, *cdoc = w.cdoc;
    CentredSoftmax sm;                               // ATTENTION
    const auto ex = [temp = a.temp](float y) { return expf(y / temp); };
    float t1 = -INFINITY, t2 = -INFINITY;           // TOP2
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    for (int c0 = 0; c0 < cl; c0 += 16) {
        const bool va = tile_row_valid(r, c0, cl);
        const float* pa = tile_row(r, cdoc + 8 * g, c0, cl);
        for (int q0 = 0; q0 < ql; q0 += 16) {
            const bool vb = tile_row_valid(r, q0, ql);
            const float* pb = tile_row(r, qdoc + 8 * g, q0, ql);
            f32x4 acc[4][4] = {{zero, zero, zero, zero}, {zero, zero, zero, zero}, {zero, zero, zero, zero}, {zero, zero, zero, zero}};
            f32x4 na = zero, nb = zero;
#pragma unroll 1
            for (int s0 = 0; s0 < kD / 32; s0 += 4) {
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int s = s0 + u;
                    const f32x4 a0 = va ? ld4(pa + 32 * s) : zero, a1 = va ? ld4(pa + 32 * s + 4) : zero;
                    const f32x4 b0 = vb ? ld4(pb + 32 * s) : zero, b1 = vb ? ld4(pb + 32 * s + 4) : zero;
                    mfma8(a0, a1, b0, b1, acc[u]);
                    na = __builtin_elementwise_fma(a1, a1, __builtin_elementwise_fma(a0, a0, na));
                    nb = __builtin_elementwise_fma(b1, b1, __builtin_elementwise_fma(b0, b0, nb));
                }
            }
            const f32x4 dot = tile_dots(acc);
            const float qn = row_sumsq(nb), cn_own = row_sumsq(na);
            float s[4], cn[4];
            bool valid[4];
#pragma unroll
            for (int v = 0; v < 4; ++v) cn[v] = __shfl(cn_own, 4 * g + v);          // (every lane: ahead of the divergent redo)
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                valid[v] = entry_valid(w, c0, v, vb);
                const float ns = qn + cn[v];
                float d2 = fmaf(-2.0f, dot[v], ns);
                if (valid[v] && expansion_cancels(d2, ns))       // (the rule: exact_d2.h)
                    d2 = exact_d2(qdoc + (int64_t)(q0 + r) * kD, cdoc + (int64_t)(c0 + 4 * g + v) * kD);
                s[v] = neg_of_expansion(d2);
            }
            if constexpr (AGG == ASPIRE_AGG_TOP2) {
#pragma unroll
                for (int v = 0; v < 4; ++v)
                    if (valid[v]) top2_merge(t1, t2, s[v], -INFINITY);
            } else {
                float tile_max = -INFINITY;
#pragma unroll
                for (int v = 0; v < 4; ++v)
                    if (valid[v]) tile_max = fmaxf(tile_max, s[v]);
                sm.raise(wave_max(tile_max), ex);
#pragma unroll
                for (int v = 0; v < 4; ++v)
                    if (valid[v]) sm.add(s[v], ex);
            }
        }
    }
    if constexpr (AGG == ASPIRE_AGG_TOP2) {
        top2_fold<1>(t1, t2);
        top2_fold<2>(t1, t2);
        top2_fold<4>(t1, t2);
        top2_fold<8>(t1, t2);
        top2_fold<16>(t1, t2);
        top2_fold<32>(t1, t2);
        if (lane == 0) a.scores[p] = t1 + (t2 == -INFINITY ? -10e8f : t2);
    } else {
        const float S = wave_sum(sm.S), T = wave_sum(sm.T);
        if (lane == 0) a.scores[p] = sm.m + T / S;
    }
}

}  // namespace
}  // namespace aspire

using namespace aspire;

extern "C" size_t aspire_l2agg_rank_batch_workspace_bytes(const aspire_repset* q, const aspire_repset* c, int64_t max_job, int64_t k) {
    return rank_scratch_only_bytes(q, c, max_job, k);
}

extern "C" int aspire_l2agg_rank_batch_f32(const aspire_repset* q, const aspire_repset* c, int64_t D, const int32_t* job_off,
                                           int64_t max_job, int cdist_mode, int agg, double temp, float* scores, int64_t k,
                                           const int32_t* job_base, float* top_scores, int64_t* top_idx, uint64_t* keys,
                                           void* workspace, size_t workspace_bytes, void* stream) {
    ASPIRE_REQUIRE(q && c, ASPIRE_ERR_INVALID_ARG, "null repset");
    {   // (the text of aspire_l2max_rank_batch_f32's limit; check_dot_sets would word it per side)
        const int max_rows = to_dot(q).bound > to_dot(c).bound ? to_dot(q).bound : to_dot(c).bound;
        ASPIRE_REQUIRE(max_rows <= generic_max_rows(), ASPIRE_ERR_UNSUPPORTED,
                       "documents with more than %d sentence rows are not supported (got %d)", generic_max_rows(), max_rows);
    }
    if (int rc = check_dot_sets(q, c, D, ASPIRE_PAIR_CROSS, ASPIRE_SIM_DOT)) return rc;
    ASPIRE_REQUIRE(agg != ASPIRE_AGG_MAX, ASPIRE_ERR_INVALID_ARG,
                   "ASPIRE_AGG_MAX over batched jobs is aspire_l2max_rank_batch_f32; this entry takes ASPIRE_AGG_TOP2 or ASPIRE_AGG_ATTENTION");
    ASPIRE_REQUIRE(agg == ASPIRE_AGG_TOP2 || agg == ASPIRE_AGG_ATTENTION, ASPIRE_ERR_INVALID_ARG, "bad aggregation %d", agg);
    ASPIRE_REQUIRE(agg != ASPIRE_AGG_ATTENTION || temp > 0, ASPIRE_ERR_INVALID_ARG, "attention temperature must be positive");
    // one formula serves AUTO / DIRECT / MM, and there is one form: ONE_FORM and CENTER have nothing to select
    cdist_mode &= ~(ASPIRE_CDIST_ONE_FORM | ASPIRE_CDIST_CENTER);
    ASPIRE_REQUIRE(cdist_mode == ASPIRE_CDIST_AUTO || cdist_mode == ASPIRE_CDIST_DIRECT || cdist_mode == ASPIRE_CDIST_MM,
                   ASPIRE_ERR_INVALID_ARG, "bad cdist_mode %d", cdist_mode);
    const int64_t J = q->n, C = c->n;
    BatchRank rank{J, max_job, k, top_scores, top_idx, keys, job_off, job_base, stream};
    bool go_on;
    if (int rc = batch_preamble(q, c, scores, rank, go_on); !go_on) return rc;
    if (int rc = place_scratch(rank, workspace, workspace_bytes, rank_scratch_only_bytes(q, c, max_job, k), 0,
                               "aspire_l2agg_rank_batch_workspace_bytes")) return rc;
    const L2aggArgs a{mapped_pair_args(q, c, job_off, scores), (float)temp};
    const auto kernel = agg == ASPIRE_AGG_TOP2 ? l2agg_pair_kernel<ASPIRE_AGG_TOP2> : l2agg_pair_kernel<ASPIRE_AGG_ATTENTION>;
    if (int rc = launch_pair_waves(kernel, a, C, (hipStream_t)stream)) return rc;
    return rank.rank(scores);
}
