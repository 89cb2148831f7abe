// Whole-document embeddings ranked by row index: the precomputed-embedding rankers (include/aspire_hip.h, A15;
// src/pre_process/pp_gen_nearest.py rank_pool :638-727 and rank_pool_faceted :1120-1199: one [N, 768] matrix of abstract reps, per
// query a pool of candidate rows, sklearn.neighbors.NearestNeighbors(algorithm='brute') per pool).
//
//   score(q, c) = L2      -sqrt(sum_k (q_k - c_k)^2)        direct differences: a candidate equal to its query scores -0.0f
//                 COSINE  <q, c> / n_q / n_c                n = sqrt(fp32 sum of squares), n < 10 * FLT_EPSILON -> 1, an infinite n
//                                                           scores 0 (dotmax.hip's rule: sklearn's float32 normalisation)
//                 DOT     <q, c>
//
// The matrix stays where it is: a job is a row index for its query and a run of row indices for its pool, nothing is copied and a
// row that sits in forty pools is stored once.  The work is one pass over 3 KB per candidate and next to no arithmetic, so the
// kernel is shaped as a gather: one wave takes a slice of kSlice consecutive candidates of the call and fetches their rows with
// 16-byte-per-lane loads (lane l owns coordinates 256 t + 4 l .. + 3, t = 0, 1, 2: a row is three 1 KiB wave loads), all kSlice
// rows issued before the first is used -- 24 KB in flight per wave.  While they fly the wave finds its job (a 64-ary search of
// job_off, one probe per lane) and loads that job's query row into registers, 12 floats per lane (from L2: the job's other waves
// read the same row).  A slice may cross a job boundary; the wave then steps to the next job and reloads the query.  Plain loads,
// not the streaming hint: pools overlap, so a candidate row is wanted again by other jobs' waves.
// One form for every call size and a fixed summation order: a lane sums its 12 terms with one fmaf chain in coordinate order, the
// 64 partial sums are added by wave_sum's fixed butterfly, and a row's squared norm is formed the same way from the row alone --
// a pair's bits depend on its two rows only, not on the job, the slice or the number of jobs.
// A row index outside [0, N) reads nothing: the lanes take zeros instead of loads and the pairs it touches score NaN.  Every other
// address is bounded by the call's own counts: cand_idx and scores by C, q_idx by J, job_off by J + 1 whatever job_off holds.
#include <float.h>
#include <math.h>

#include "common.h"
#include "batch_host.h"
#include "dot_tiles.h"

namespace aspire {
namespace {

constexpr int kSlice = 8;       // candidates per wave, all in flight at once
constexpr int kT = kD / 256;    // 16-byte pieces of a row per lane

struct DenseArgs {
    const float* rows;          // [N, 768]
    int64_t N;
    const int32_t* q_idx;       // [J]
    const int32_t* cand_idx;    // [C]
    const int32_t* job_off;     // [J + 1]
    int32_t J;
    int64_t C;
    float* scores;              // [C]
};

struct Row {
    f32x4 v[kT];
};

// row `idx` of the matrix as the lane's 12 coordinates.  CHECKED: `ok` false (an index outside [0, N)) reads nothing
template <bool CHECKED>
__device__ __forceinline__ Row load_row(const float* rows, int32_t idx, bool ok, int lane) {
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    const float* p = rows + (int64_t)(!CHECKED || ok ? idx : 0) * kD + 4 * lane;
    Row r;
#pragma unroll
    for (int t = 0; t < kT; ++t) r.v[t] = !CHECKED || ok ? ld4(p + 256 * t) : zero;
    return r;
}

// the lane's share of <x, y>: one chain over its 12 coordinates in ascending order
__device__ __forceinline__ float dot12(const Row& x, const Row& y) {
    float s = 0.f;
#pragma unroll
    for (int t = 0; t < kT; ++t) {
        s = fmaf(x.v[t].x, y.v[t].x, s);
        s = fmaf(x.v[t].y, y.v[t].y, s);
        s = fmaf(x.v[t].z, y.v[t].z, s);
        s = fmaf(x.v[t].w, y.v[t].w, s);
    }
    return s;
}

__device__ __forceinline__ float diff12(const Row& x, const Row& y) {
    float s = 0.f;
#pragma unroll
    for (int t = 0; t < kT; ++t) {
        const f32x4 d = x.v[t] - y.v[t];
        s = fmaf(d.x, d.x, s);
        s = fmaf(d.y, d.y, s);
        s = fmaf(d.z, d.z, s);
        s = fmaf(d.w, d.w, s);
    }
    return s;
}

// sklearn's row norm: sqrt of the fp32 sum of squares, near-zero -> 1 (dotmax.hip)
__device__ __forceinline__ float row_norm(float ss) {
    const float n = sqrtf(ss);
    return n < 10.0f * FLT_EPSILON ? 1.0f : n;
}

// dot_tiles.h's job_of (the last j with job_off[j] <= p) as a 64-ary search: one probe per lane and level, so 50 jobs are one
// round trip and 4096 two.  Only job_off[1 .. J - 1] is read and the result is in [0, J), whatever the table holds.
__device__ __forceinline__ int32_t job_of_wave(const int32_t* __restrict__ job_off, int32_t J, int64_t p, int lane) {
    int32_t lo = 0, hi = J;          // invariant: job_off[lo] <= p < job_off[hi]
    while (hi - lo > 1) {
        const int32_t step = (hi - lo + 63) / 64;
        const int32_t m = lo + (lane + 1) * step;
        const bool le = m < hi && job_off[m] <= p;
        lo += __popcll(__ballot(le)) * step;        // job_off is non-decreasing: the probes that hold are the first ones
        hi = hi < lo + step ? hi : lo + step;
    }
    return lo;
}

template <int METRIC>
__global__ void __launch_bounds__(256) dense_rank_kernel(DenseArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t p0 = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * kSlice;
    if (p0 >= a.C) return;
    const int n = a.C - p0 < kSlice ? (int)(a.C - p0) : kSlice;        // candidates of this slice
    // the slice's row indices: one load, lane u holds candidate u's
    const int32_t my_ci = lane < n ? a.cand_idx[p0 + lane] : -1;
    int32_t ci[kSlice];
    bool ok[kSlice], all_ok = true;
#pragma unroll
    for (int u = 0; u < kSlice; ++u) {
        ci[u] = __builtin_amdgcn_readlane(my_ci, u);
        ok[u] = ci[u] >= 0 && ci[u] < a.N;
        all_ok = all_ok && ok[u];
    }
    Row c[kSlice];
    if (all_ok) {                       // (wave-uniform, as every branch of this kernel) a full slice of good rows: no test per load
#pragma unroll
        for (int u = 0; u < kSlice; ++u) c[u] = load_row<false>(a.rows, ci[u], true, lane);
    } else {
#pragma unroll
        for (int u = 0; u < kSlice; ++u) c[u] = load_row<true>(a.rows, ci[u], ok[u], lane);
    }
    int32_t j = job_of_wave(a.job_off, a.J, p0, lane);
    int64_t jend = p0;                  // job_off[j + 1] once the query is loaded
    Row q;
    bool q_ok = false;
    float nq = 1.0f;                    // COSINE: the query's norm
#pragma unroll
    for (int u = 0; u < kSlice; ++u) {
        const int64_t p = p0 + u;
        if (u >= n) break;
        if (u == 0 || p >= jend) {
            if (u > 0 && j + 1 < a.J) ++j;
            while (j + 1 < a.J && a.job_off[j + 1] <= p) ++j;          // (empty jobs)
            jend = a.job_off[j + 1];
            const int32_t qi = a.q_idx[j];
            q_ok = qi >= 0 && qi < a.N;
            q = load_row<true>(a.rows, qi, q_ok, lane);
            if constexpr (METRIC == ASPIRE_DENSE_COSINE) nq = row_norm(wave_sum(dot12(q, q)));
        }
        float s;
        if constexpr (METRIC == ASPIRE_DENSE_L2) {
            s = -sqrtf(wave_sum(diff12(q, c[u])));
        } else {
            s = wave_sum(dot12(q, c[u]));
            if constexpr (METRIC == ASPIRE_DENSE_COSINE) {
                const float nc = row_norm(wave_sum(dot12(c[u], c[u])));
                s = isinf(nq) || isinf(nc) ? 0.0f : s / nq / nc;        // x / inf = 0 row: no inf / inf
            }
        }
        if (lane == 0) a.scores[p] = q_ok && ok[u] ? s : __builtin_nanf("");
    }
}

int launch_dense(const DenseArgs& a, int metric, hipStream_t s) {
    const int64_t blocks = (a.C + 4 * kSlice - 1) / (4 * kSlice);
    ASPIRE_REQUIRE(blocks < ((int64_t)1 << 31), ASPIRE_ERR_UNSUPPORTED, "too many pairs: %lld", (long long)a.C);
    const dim3 grid((unsigned)blocks), block(256);
    if (metric == ASPIRE_DENSE_L2) hipLaunchKernelGGL(dense_rank_kernel<ASPIRE_DENSE_L2>, grid, block, 0, s, a);
    else if (metric == ASPIRE_DENSE_COSINE) hipLaunchKernelGGL(dense_rank_kernel<ASPIRE_DENSE_COSINE>, grid, block, 0, s, a);
    else hipLaunchKernelGGL(dense_rank_kernel<ASPIRE_DENSE_DOT>, grid, block, 0, s, a);
    ASPIRE_LAUNCH_OK();
    return ASPIRE_OK;
}

}  // namespace
}  // namespace aspire

using namespace aspire;

extern "C" size_t aspire_dense_rank_batch_workspace_bytes(int64_t J, int64_t C, int64_t max_job, int64_t k) {
    return rank_scratch_only_bytes(J, C, max_job, k);
}

extern "C" int aspire_dense_rank_batch_f32(const float* rows, int64_t N, int64_t D, const int32_t* q_idx, int64_t J,
                                           const int32_t* cand_idx, int64_t C, const int32_t* job_off, int64_t max_job, int metric,
                                           float* scores, int64_t k, const int32_t* job_base, float* top_scores, int64_t* top_idx,
                                           uint64_t* keys, void* workspace, size_t workspace_bytes, void* stream) {
    ASPIRE_REQUIRE(D == kD, ASPIRE_ERR_UNSUPPORTED, "encoding dim %lld unsupported (kernels are built for 768)", (long long)D);
    ASPIRE_REQUIRE(metric == ASPIRE_DENSE_L2 || metric == ASPIRE_DENSE_COSINE || metric == ASPIRE_DENSE_DOT, ASPIRE_ERR_INVALID_ARG,
                   "bad metric %d", metric);
    ASPIRE_REQUIRE(N >= 0 && J >= 0 && C >= 0, ASPIRE_ERR_INVALID_ARG, "negative row / job / candidate count");
    ASPIRE_REQUIRE(N < ((int64_t)1 << 31), ASPIRE_ERR_UNSUPPORTED, "row indices are 32-bit: %lld rows", (long long)N);
    // the siblings' preamble takes its counts from two rep sets: CSR sets of J and C documents stand in for the index lists
    aspire_repset qs{}, cs{};
    qs.n = J;
    cs.n = C;
    BatchRank rank{J, max_job, k, top_scores, top_idx, keys, job_off, job_base, stream};
    bool go_on;
    if (int rc = batch_preamble(&qs, &cs, scores, rank, go_on); !go_on) return rc;
    ASPIRE_REQUIRE(q_idx && cand_idx, ASPIRE_ERR_INVALID_ARG, "null q_idx / cand_idx");
    ASPIRE_REQUIRE(rows || N == 0, ASPIRE_ERR_INVALID_ARG, "null rows");
    ASPIRE_REQUIRE(((uintptr_t)rows & 15) == 0, ASPIRE_ERR_INVALID_ARG, "rows must be 16-byte aligned");
    if (int rc = place_scratch(rank, workspace, workspace_bytes, rank_scratch_only_bytes(J, C, max_job, k), 0,
                               "aspire_dense_rank_batch_workspace_bytes")) return rc;
    const DenseArgs a{rows, N, q_idx, cand_idx, job_off, (int32_t)J, C, scores};
    if (int rc = launch_dense(a, metric, (hipStream_t)stream)) return rc;
    return rank.rank(scores);
}
