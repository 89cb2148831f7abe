// The operand and product helpers of the kernels that form sentence-pair dot products on v_mfma_f32_16x16x4_f32 (dotmax.hip: max over
// the block; jointsm.hip: joint soft-max over the block; l2agg_pair.hip: top-2 / soft-max of the negated L2 distances): the rep-set view
// the kernels read, the operand loads, the eight-k product step and the sum of squares beside it, the job lookup of the batched form,
// and the host-side set check.  The frame around them -- which wave works on which pair, the tile walk, the cross kernels' row slots,
// the launchers -- is pair_fwd.h, which includes this file.  A lane holds A[row l & 15][k] and B[k][col l & 15] for
// k = 32 s + 8 (l >> 4) + e: the k order inside a block of 32 is permuted identically for both operands, so the sums are the
// same dot products -- and the same bits in every kernel that spreads the k blocks over its accumulators the same way (the two
// kernels of dotmax.hip: four accumulators; the two of jointsm.hip and l2agg_pair.hip's: sixteen).
#pragma once
#include "common.h"

namespace aspire {
int generic_max_rows(void);

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kModeCross = 0, kModePaired = 1, kModeMapped = 2;
constexpr int kXRows = 32;              // candidate row slots per cross workgroup
constexpr int kXStride = kD + 4;        // LDS row stride (floats): rows 16 B apart in the banks

struct DotSet {
    const float* rows;
    const int32_t* start;
    const int32_t* len;
    int64_t n;
    int32_t bound;      // host-known upper bound of len[] (ext, or max_len): a longer document scores NaN
};

__device__ __forceinline__ f32x4 ld4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }

__device__ __forceinline__ f32x4 mfma4(float a, float b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

// eight k values of one row against eight of one column into acc[0..3] (k = e spread over the four accumulators)
__device__ __forceinline__ void mfma8(const f32x4& a0, const f32x4& a1, const f32x4& b0, const f32x4& b1, f32x4 (&acc)[4]) {
    acc[0] = mfma4(a0.x, b0.x, acc[0]);
    acc[1] = mfma4(a0.y, b0.y, acc[1]);
    acc[2] = mfma4(a0.z, b0.z, acc[2]);
    acc[3] = mfma4(a0.w, b0.w, acc[3]);
    acc[0] = mfma4(a1.x, b1.x, acc[0]);
    acc[1] = mfma4(a1.y, b1.y, acc[1]);
    acc[2] = mfma4(a1.z, b1.z, acc[2]);
    acc[3] = mfma4(a1.w, b1.w, acc[3]);
}

// eight more squares onto a row's sum of squares, in the operands' order (dotmax.hip's norms)
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

// a tile's dot products from sixteen accumulators (jointsm.hip, l2agg_pair.hip; set u: k blocks s = u mod 4)
__device__ __forceinline__ f32x4 tile_dots(const f32x4 (&acc)[4][4]) {
    f32x4 t[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) t[u] = (acc[u][0] + acc[u][1]) + (acc[u][2] + acc[u][3]);
    return (t[0] + t[1]) + (t[2] + t[3]);
}

// job of candidate p: the last j with job_off[j] <= p (empty jobs skipped)
__device__ __forceinline__ int32_t job_of(const int32_t* __restrict__ job_off, int32_t J, int64_t p) {
    int32_t lo = 0, hi = J;          // invariant: job_off[lo] <= p < job_off[hi]
    while (hi - lo > 1) {
        const int32_t mid = (lo + hi) >> 1;
        if (job_off[mid] <= p) lo = mid; else hi = mid;
    }
    return lo;
}

DotSet to_dot(const aspire_repset* s) {
    return DotSet{s->rows, s->start, s->len, s->n, s->ext > 0 ? s->ext : s->max_len};
}

int check_dot_sets(const aspire_repset* q, const aspire_repset* c, int64_t D, int pairing, int sim) {
    ASPIRE_REQUIRE(q && c, ASPIRE_ERR_INVALID_ARG, "null repset");
    ASPIRE_REQUIRE(D == kD, ASPIRE_ERR_UNSUPPORTED, "encoding dim %lld unsupported (kernels are built for 768)", (long long)D);
    ASPIRE_REQUIRE(pairing == ASPIRE_PAIR_CROSS || pairing == ASPIRE_PAIR_PAIRED, ASPIRE_ERR_INVALID_ARG, "bad pairing %d", pairing);
    ASPIRE_REQUIRE(sim == ASPIRE_SIM_COSINE || sim == ASPIRE_SIM_DOT, ASPIRE_ERR_INVALID_ARG, "bad similarity %d", sim);
    ASPIRE_REQUIRE(q->n >= 0 && c->n >= 0, ASPIRE_ERR_INVALID_ARG, "negative document count");
    ASPIRE_REQUIRE(pairing != ASPIRE_PAIR_PAIRED || q->n == c->n, ASPIRE_ERR_INVALID_ARG,
                   "paired scoring needs equal batch sizes (query %lld vs cand %lld)", (long long)q->n, (long long)c->n);
    ASPIRE_REQUIRE(q->ext >= 0 && c->ext >= 0 && q->max_len >= 0 && c->max_len >= 0, ASPIRE_ERR_INVALID_ARG, "negative ext / max_len");
    const int bq = to_dot(q).bound, bc = to_dot(c).bound;
    ASPIRE_REQUIRE(bq <= generic_max_rows() && bc <= generic_max_rows(), ASPIRE_ERR_UNSUPPORTED,
                   "documents with more than %d sentence rows are not supported (got %d x %d)", generic_max_rows(), bq, bc);
    if (q->n == 0 || c->n == 0) return ASPIRE_OK;
    ASPIRE_REQUIRE(q->rows && q->start && q->len && c->rows && c->start && c->len, ASPIRE_ERR_INVALID_ARG, "null rows / start / len");
    ASPIRE_REQUIRE(((uintptr_t)q->rows & 15) == 0 && ((uintptr_t)c->rows & 15) == 0, ASPIRE_ERR_INVALID_ARG,
                   "rows must be 16-byte aligned");
    return ASPIRE_OK;
}

}  // namespace
}  // namespace aspire
