// The supervised-alignment distances (include/aspire_hip.h, aspire_l2sup_scores_f32 / aspire_l2sup_backward_f32): the L2 distance of
// ONE pre-aligned (query sentence, candidate sentence) per pair -- allpair_masked_dist_l2sup and allpair_masked_dist_l2sup_weighted
// (pair_distances.py:189-292), the criterion_sentsup of WordSentAbsSupAlignBiEnc (disent_models.py:704-710, :818).
//
//   align[p] = (a0, a1):  i = min(a0, q_len - 1),  j = min(a1, c_len - 1)       (the reference's clipping, :214-215)
//   similarity = -d,  d = ||q_i - c_j|| from the DIRECT difference;  weighted: divided by (float)(q_len * c_len)   (:264, :290)
//   backward through torch.cdist's rule:  grad_q_i = -g (q_i - c_j) / d,  grad_c_j = +g (q_i - c_j) / d,  both 0 where d == 0;
//   every other row of the two documents gets exact zeros, pad rows (len <= r < ext) included.
// The reference forms the whole -cdist block and reads one entry; here only that entry is formed.  A negative index (the host layer
// raises on it) reads nothing: the pair's score is NaN and so are its valid gradient rows.  A document longer than its set's
// host-known bound is poisoned the same way, as in the other kernels.
//   l2sup_fwd_kernel   one wave per pair: two rows, one wave_sum.
//   l2sup_bwd_kernel   pair_bwd.h's frame with the pick given instead of found (every wave forms the one difference itself: no
//                      LDS, no barrier).
#include "pair_bwd.h"

namespace aspire {
namespace {

struct L2SupArgs {
    RepSet q, c;
    const int32_t* align;       // [P, 2]
    int weighted;
    float* scores;              // forward
    const float* grad_scores;   // backward
    float* grad_q;
    float* grad_c;
};

__global__ void __launch_bounds__(kPairBwdThreads) l2sup_fwd_kernel(L2SupArgs a, int64_t P, int rows_q, int rows_c) {
    const int lane = threadIdx.x & 63;
    const int64_t p = (int64_t)blockIdx.x * kPairBwdWaves + (threadIdx.x >> 6);
    if (p >= P) return;
    const int q_len = a.q.len[p], c_len = a.c.len[p], a0 = a.align[2 * p], a1 = a.align[2 * p + 1];
    if (q_len > rows_q || c_len > rows_c || q_len <= 0 || c_len <= 0 || a0 < 0 || a1 < 0) {         // (wave-uniform)
        if (lane == 0) a.scores[p] = __builtin_nanf("");
        return;
    }
    const int i = a0 < q_len - 1 ? a0 : q_len - 1, j = a1 < c_len - 1 ? a1 : c_len - 1;
    const Row x = load_row(a.q.rows + ((size_t)a.q.start[p] + i) * kD, lane);
    const Row y = load_row(a.c.rows + ((size_t)a.c.start[p] + j) * kD, lane);
    float s = -row_length(diff(x, y));
    if (a.weighted) s = s / (float)(q_len * c_len);
    if (lane == 0) a.scores[p] = s;
}

__global__ void __launch_bounds__(kPairBwdThreads) l2sup_bwd_kernel(L2SupArgs a, int rows_q, int rows_c) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t p = blockIdx.x;
    const int a0 = a.align[2 * p], a1 = a.align[2 * p + 1];
    PairFrame f = pair_frame(a.q, a.c, a.grad_q, a.grad_c, p, rows_q, rows_c);
    f.poison = f.poison || a0 < 0 || a1 < 0;
    if (skip_pair(f, lane, wave)) return;
    const int ql = f.ql, cl = f.cl;
    const int i = a0 < ql - 1 ? a0 : ql - 1, j = a1 < cl - 1 ? a1 : cl - 1;
    const Row e = diff(load_row(f.qdoc + (size_t)i * kD, lane), load_row(f.cdoc + (size_t)j * kD, lane));
    const float d = row_length(e);
    const float g = a.grad_scores[p];
    const Row unit = scaled(d > 0.f ? 1.0f / d : 0.f, e);          // (q_i - c_j) / d; 0 for coincident rows (torch.cdist's rule)
    Row row_q = scaled(-g, unit), row_c = scaled(g, unit);
    if (a.weighted) {          // the plain form's rows over the block size: one more rounding, as in the forward
        const float n = (float)(ql * cl);
        row_q = Row{row_q.x / n, row_q.y / n, row_q.z / n};
        row_c = Row{row_c.x / n, row_c.y / n, row_c.z / n};
    }
    const Row zero = splat(0.f);
    for (int r = wave; r < f.q_own; r += kPairBwdWaves) store_row(f.gq + (size_t)r * kD, lane, r == i ? row_q : zero);
    for (int r = wave; r < f.c_own; r += kPairBwdWaves) store_row(f.gc + (size_t)r * kD, lane, r == j ? row_c : zero);
}

}  // namespace

// One wave per pair of `q` / `c` (PAIRED: q.n == c.n); rows_q / rows_c: host-known bounds of the documents' rows.
int launch_l2sup_scores(const RepSet& q, const RepSet& c, const int32_t* align, int weighted, float* scores, int rows_q, int rows_c,
                        hipStream_t stream) {
    if (int rc = check_row_bounds(rows_q, rows_c)) return rc;
    const int64_t P = c.n;
    if (P == 0) return ASPIRE_OK;
    const int64_t blocks = (P + kPairBwdWaves - 1) / kPairBwdWaves;
    ASPIRE_REQUIRE(blocks < ((int64_t)1 << 31), ASPIRE_ERR_UNSUPPORTED, "too many pairs: %lld", (long long)P);
    L2SupArgs a{q, c, align, weighted, scores, nullptr, nullptr, nullptr};
    hipLaunchKernelGGL(l2sup_fwd_kernel, dim3((unsigned)blocks), dim3(kPairBwdThreads), 0, stream, a, P, rows_q, rows_c);
    ASPIRE_LAUNCH_OK();
    return ASPIRE_OK;
}

// One workgroup per pair; grad_q / grad_c are laid out like q.rows / c.rows.
int launch_l2sup_backward(const RepSet& q, const RepSet& c, const int32_t* align, int weighted, const float* grad_scores, float* grad_q,
                          float* grad_c, int rows_q, int rows_c, hipStream_t stream) {
    return launch_pair_bwd(l2sup_bwd_kernel, L2SupArgs{q, c, align, weighted, nullptr, grad_scores, grad_q, grad_c}, c.n, 0, 0, rows_q, rows_c,
                           stream);
}

}  // namespace aspire
