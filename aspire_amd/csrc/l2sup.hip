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
//   l2sup_bwd_kernel   l2agg_bwd.hip's frame with the pick given instead of found: one workgroup of four waves per pair, a lane owns
//                      12 of the 768 coordinates, wave w writes rows w, w + 4, ... once with 16-byte stores (every wave forms the
//                      one difference itself: no LDS, no barrier).  No atomics: the same bits on every run.
#include <math.h>

#include "common.h"
#include "score_types.h"

namespace aspire {
namespace {

constexpr int kSupThreads = 256, kSupWaves = kSupThreads / 64;

typedef float v4 __attribute__((ext_vector_type(4)));
struct Row {          // a lane's 12 coordinates of one row: 4 lane + 256 k + (0 .. 3)
    v4 x, y, z;
};
__device__ __forceinline__ Row load_row(const float* row, int lane) {
    const v4* p = reinterpret_cast<const v4*>(row) + lane;
    return Row{p[0], p[64], p[128]};
}
__device__ __forceinline__ void store_row(float* row, int lane, const Row& r) {
    v4* p = reinterpret_cast<v4*>(row) + lane;
    p[0] = r.x;
    p[64] = r.y;
    p[128] = r.z;
}
__device__ __forceinline__ Row splat(float v) { return Row{v4{v, v, v, v}, v4{v, v, v, v}, v4{v, v, v, v}}; }
__device__ __forceinline__ Row diff(const Row& a, const Row& b) { return Row{a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ Row scaled(float f, const Row& r) { return Row{f * r.x, f * r.y, f * r.z}; }
// ||e|| of a row spread over the wave
__device__ __forceinline__ float row_norm(const Row& e) {
    const v4 sq = __builtin_elementwise_fma(e.z, e.z, __builtin_elementwise_fma(e.y, e.y, e.x * e.x));
    return sqrtf(wave_sum((sq.x + sq.y) + (sq.z + sq.w)));
}

struct L2SupArgs {
    RepSet q, c;
    const int32_t* align;       // [P, 2]
    int weighted;
    float* scores;              // forward
    const float* grad_scores;   // backward
    float* grad_q;
    float* grad_c;
};

__global__ void __launch_bounds__(kSupThreads) l2sup_fwd_kernel(L2SupArgs a, int64_t P, int rows_q, int rows_c) {
    const int lane = threadIdx.x & 63;
    const int64_t p = (int64_t)blockIdx.x * kSupWaves + (threadIdx.x >> 6);
    if (p >= P) return;
    const int q_len = a.q.len[p], c_len = a.c.len[p], a0 = a.align[2 * p], a1 = a.align[2 * p + 1];
    if (q_len > rows_q || c_len > rows_c || q_len <= 0 || c_len <= 0 || a0 < 0 || a1 < 0) {         // (wave-uniform)
        if (lane == 0) a.scores[p] = __builtin_nanf("");
        return;
    }
    const int i = a0 < q_len - 1 ? a0 : q_len - 1, j = a1 < c_len - 1 ? a1 : c_len - 1;
    const Row x = load_row(a.q.rows + ((size_t)a.q.start[p] + i) * kD, lane);
    const Row y = load_row(a.c.rows + ((size_t)a.c.start[p] + j) * kD, lane);
    float s = -row_norm(diff(x, y));
    if (a.weighted) s = s / (float)(q_len * c_len);
    if (lane == 0) a.scores[p] = s;
}

__global__ void __launch_bounds__(kSupThreads) l2sup_bwd_kernel(L2SupArgs a, int rows_q, int rows_c) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t p = blockIdx.x;
    const int q_len = a.q.len[p], c_len = a.c.len[p], a0 = a.align[2 * p], a1 = a.align[2 * p + 1];
    const bool poison = q_len > rows_q || c_len > rows_c || a0 < 0 || a1 < 0;
    const int ql = q_len < 0 ? 0 : (q_len > rows_q ? rows_q : q_len), cl = c_len < 0 ? 0 : (c_len > rows_c ? rows_c : c_len);
    const int q_own = a.q.ext > 0 ? a.q.ext : ql, c_own = a.c.ext > 0 ? a.c.ext : cl;        // rows this pair writes (pad rows included)
    const float* qdoc = a.q.rows + (size_t)a.q.start[p] * kD;
    const float* cdoc = a.c.rows + (size_t)a.c.start[p] * kD;
    float* gq = a.grad_q + (size_t)a.q.start[p] * kD;
    float* gc = a.grad_c + (size_t)a.c.start[p] * kD;
    if (poison || ql * cl == 0) {             // (workgroup-uniform)
        const float v = poison ? __builtin_nanf("") : 0.f;
        for (int r = wave; r < q_own; r += kSupWaves) store_row(gq + (size_t)r * kD, lane, splat(r < ql ? v : 0.f));
        for (int r = wave; r < c_own; r += kSupWaves) store_row(gc + (size_t)r * kD, lane, splat(r < cl ? v : 0.f));
        return;
    }
    const int i = a0 < ql - 1 ? a0 : ql - 1, j = a1 < cl - 1 ? a1 : cl - 1;
    const Row e = diff(load_row(qdoc + (size_t)i * kD, lane), load_row(cdoc + (size_t)j * kD, lane));
    const float d = row_norm(e);
    const float g = a.grad_scores[p];
    const Row unit = scaled(d > 0.f ? 1.0f / d : 0.f, e);          // (q_i - c_j) / d; 0 for coincident rows (torch.cdist's rule)
    Row row_q = scaled(-g, unit), row_c = scaled(g, unit);
    if (a.weighted) {          // the plain form's rows over the block size: one more rounding, as in the forward
        const float n = (float)(ql * cl);
        row_q = Row{row_q.x / n, row_q.y / n, row_q.z / n};
        row_c = Row{row_c.x / n, row_c.y / n, row_c.z / n};
    }
    const Row zero = splat(0.f);
    for (int r = wave; r < q_own; r += kSupWaves) store_row(gq + (size_t)r * kD, lane, r == i ? row_q : zero);
    for (int r = wave; r < c_own; r += kSupWaves) store_row(gc + (size_t)r * kD, lane, r == j ? row_c : zero);
}

int check_rows(int rows_q, int rows_c) {
    ASPIRE_REQUIRE(rows_q <= generic_max_rows() && rows_c <= generic_max_rows(), ASPIRE_ERR_UNSUPPORTED,
                   "documents with more than %d sentence rows are not supported (got %d x %d)", generic_max_rows(), rows_q, rows_c);
    return ASPIRE_OK;
}

}  // namespace

// One wave per pair of `q` / `c` (PAIRED: q.n == c.n); rows_q / rows_c: host-known bounds of the documents' rows.
int launch_l2sup_scores(const RepSet& q, const RepSet& c, const int32_t* align, int weighted, float* scores, int rows_q, int rows_c,
                        hipStream_t stream) {
    if (int rc = check_rows(rows_q, rows_c)) return rc;
    const int64_t P = c.n;
    if (P == 0) return ASPIRE_OK;
    const int64_t blocks = (P + kSupWaves - 1) / kSupWaves;
    ASPIRE_REQUIRE(blocks < ((int64_t)1 << 31), ASPIRE_ERR_UNSUPPORTED, "too many pairs: %lld", (long long)P);
    L2SupArgs a{q, c, align, weighted, scores, nullptr, nullptr, nullptr};
    hipLaunchKernelGGL(l2sup_fwd_kernel, dim3((unsigned)blocks), dim3(kSupThreads), 0, stream, a, P, rows_q, rows_c);
    ASPIRE_LAUNCH_OK();
    return ASPIRE_OK;
}

// One workgroup per pair; grad_q / grad_c are laid out like q.rows / c.rows.
int launch_l2sup_backward(const RepSet& q, const RepSet& c, const int32_t* align, int weighted, const float* grad_scores, float* grad_q,
                          float* grad_c, int rows_q, int rows_c, hipStream_t stream) {
    if (int rc = check_rows(rows_q, rows_c)) return rc;
    const int64_t P = c.n;
    if (P == 0) return ASPIRE_OK;
    ASPIRE_REQUIRE(P < ((int64_t)1 << 31), ASPIRE_ERR_UNSUPPORTED, "too many pairs: %lld", (long long)P);
    L2SupArgs a{q, c, align, weighted, nullptr, grad_scores, grad_q, grad_c};
    hipLaunchKernelGGL(l2sup_bwd_kernel, dim3((unsigned)P), dim3(kSupThreads), 0, stream, a, rows_q, rows_c);
    ASPIRE_LAUNCH_OK();
    return ASPIRE_OK;
}

}  // namespace aspire
