// The frame the backward kernels of the sentence-pair distances share (l2agg_bwd.hip, ot_bwd.hip, jointsm_bwd.hip, l2sup.hip): what a
// pair's workgroup owns and writes, apart from the distance's own mathematics.
//
// One workgroup of four waves per pair (ASPIRE_PAIR_PAIRED: every document belongs to one pair, so a gradient row has one writer --
// no atomics, nothing summed across workgroups, the same bits on every run).  A lane owns 12 of a row's 768 coordinates (three
// 16-byte pieces, 1 KiB per wave-instruction), a wave the rows r = wave, wave + 4, ...  Every row the pair owns is written once, by
// the lanes that own its coordinates, with 16-byte vector stores.
//   poison    a document longer than its set's host-known bound (rows_q / rows_c) has its rows, up to the bound, set to NaN, and so
//             has its partner, as the forward poisons the pair's score; a kernel may add causes of its own (l2sup.hip: a negative
//             alignment index) before it asks skip_pair.
//   empty     a pair with a document of no rows has no gradient: the other document's rows get exact zeros.
//   pad rows  of padded sets (len <= r < ext) get exact zeros in every case; CSR sets (ext == 0) own their valid rows only.
// The host side: one launcher for the four kernels (row bound, pair count, dynamic LDS beyond 64 KiB, one workgroup per pair).
#pragma once
#include <math.h>

#include "common.h"
#include "score_types.h"

namespace aspire {

constexpr int kPairBwdThreads = 256, kPairBwdWaves = kPairBwdThreads / 64;

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
// acc += w (a - b)
__device__ __forceinline__ void add_diff(Row& acc, float w, const Row& a, const Row& b) {
    const v4 ww = {w, w, w, w};
    acc.x = __builtin_elementwise_fma(ww, a.x - b.x, acc.x);
    acc.y = __builtin_elementwise_fma(ww, a.y - b.y, acc.y);
    acc.z = __builtin_elementwise_fma(ww, a.z - b.z, acc.z);
}
// acc += w a
__device__ __forceinline__ void add_scaled(Row& acc, float w, const Row& a) {
    const v4 ww = {w, w, w, w};
    acc.x = __builtin_elementwise_fma(ww, a.x, acc.x);
    acc.y = __builtin_elementwise_fma(ww, a.y, acc.y);
    acc.z = __builtin_elementwise_fma(ww, a.z, acc.z);
}
// ||e|| of a row spread over the wave
__device__ __forceinline__ float row_length(const Row& e) {
    const v4 sq = __builtin_elementwise_fma(e.z, e.z, __builtin_elementwise_fma(e.y, e.y, e.x * e.x));
    return sqrtf(wave_sum((sq.x + sq.y) + (sq.z + sq.w)));
}

// the four waves' sums / maxima in one fixed order (every thread calls; `red` = 4 floats)
__device__ __forceinline__ float block_sum4(float v, float* red) {
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    const float r = (red[0] + red[1]) + (red[2] + red[3]);
    __syncthreads();
    return r;
}
__device__ __forceinline__ float block_max4(float v, float* red) {
    v = wave_max(v);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    const float r = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    __syncthreads();
    return r;
}

struct PairFrame {
    int ql, cl;                     // valid rows, clamped to [0, the host-known bound]
    int q_own, c_own;               // rows this pair writes (pad rows included)
    const float *qdoc, *cdoc;       // the pair's documents
    float *gq, *gc;                 // and their gradient rows, laid out alike
    bool poison;                    // longer than the host-known bound
};
__device__ __forceinline__ PairFrame pair_frame(const RepSet& q, const RepSet& c, float* grad_q, float* grad_c, int64_t p, int rows_q,
                                                int rows_c) {
    const int q_len = q.len[p], c_len = c.len[p];
    PairFrame f;
    f.poison = q_len > rows_q || c_len > rows_c;
    f.ql = q_len < 0 ? 0 : (q_len > rows_q ? rows_q : q_len);
    f.cl = c_len < 0 ? 0 : (c_len > rows_c ? rows_c : c_len);
    f.q_own = q.ext > 0 ? q.ext : f.ql;
    f.c_own = c.ext > 0 ? c.ext : f.cl;
    f.qdoc = q.rows + (size_t)q.start[p] * kD;
    f.cdoc = c.rows + (size_t)c.start[p] * kD;
    f.gq = grad_q + (size_t)q.start[p] * kD;
    f.gc = grad_c + (size_t)c.start[p] * kD;
    return f;
}
// A poisoned or empty pair: its rows are written here (NaN or zero; pad rows zero) and the caller returns.  Workgroup-uniform.
__device__ __forceinline__ bool skip_pair(const PairFrame& f, int lane, int wave) {
    if (!f.poison && f.ql * f.cl != 0) return false;
    const float v = f.poison ? __builtin_nanf("") : 0.f;
    for (int r = wave; r < f.q_own; r += kPairBwdWaves) store_row(f.gq + (size_t)r * kD, lane, splat(r < f.ql ? v : 0.f));
    for (int r = wave; r < f.c_own; r += kPairBwdWaves) store_row(f.gc + (size_t)r * kD, lane, splat(r < f.cl ? v : 0.f));
    return true;
}
__device__ __forceinline__ void zero_pad_rows(const PairFrame& f, int lane, int wave) {
    const Row zero = splat(0.f);
    for (int r = f.ql + wave; r < f.q_own; r += kPairBwdWaves) store_row(f.gq + (size_t)r * kD, lane, zero);
    for (int r = f.cl + wave; r < f.c_own; r += kPairBwdWaves) store_row(f.gc + (size_t)r * kD, lane, zero);
}
// d_ij = ||q_i - c_j|| from the DIRECT differences into dist[i * ld + j] over the valid block, one wave_sum per entry (the caller's
// barrier publishes them)
__device__ __forceinline__ void direct_distances(const PairFrame& f, float* dist, int ld, int lane, int wave) {
    for (int i = wave; i < f.ql; i += kPairBwdWaves) {
        const Row x = load_row(f.qdoc + (size_t)i * kD, lane);
        for (int j = 0; j < f.cl; ++j) {
            const Row y = load_row(f.cdoc + (size_t)j * kD, lane);
            const v4 e0 = x.x - y.x, e1 = x.y - y.y, e2 = x.z - y.z;
            const v4 sq = __builtin_elementwise_fma(e2, e2, __builtin_elementwise_fma(e1, e1, e0 * e0));
            const float d2 = wave_sum((sq.x + sq.y) + (sq.z + sq.w));
            if (lane == 0) dist[i * ld + j] = sqrtf(d2);
        }
    }
}

// rows_q / rows_c: host-known bounds of the documents' rows
inline int check_row_bounds(int rows_q, int rows_c) {
    ASPIRE_REQUIRE(rows_q <= generic_max_rows() && rows_c <= generic_max_rows(), ASPIRE_ERR_UNSUPPORTED,
                   "documents with more than %d sentence rows are not supported (got %d x %d)", generic_max_rows(), rows_q, rows_c);
    return ASPIRE_OK;
}
// One workgroup per pair, P pairs: kernel(args, rows_q, rows_c) with lds_bytes of dynamic LDS (lds_cap_bytes: what rows at the bound
// need at most)
template <class Args>
int launch_pair_bwd(void (*kernel)(Args, int, int), const Args& args, int64_t P, size_t lds_bytes, int lds_cap_bytes, int rows_q, int rows_c,
                    hipStream_t stream) {
    if (int rc = check_row_bounds(rows_q, rows_c)) return rc;
    if (P == 0) return ASPIRE_OK;
    ASPIRE_REQUIRE(P < ((int64_t)1 << 31), ASPIRE_ERR_UNSUPPORTED, "too many pairs: %lld", (long long)P);
    if (lds_bytes > 64 * 1024) {      // more than the default dynamic LDS limit: raise it (per function, sticky, harmless to repeat)
        ASPIRE_HIP_OK(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, lds_cap_bytes));
    }
    hipLaunchKernelGGL(kernel, dim3((unsigned)P), dim3(kPairBwdThreads), lds_bytes, stream, args, rows_q, rows_c);
    ASPIRE_LAUNCH_OK();
    return ASPIRE_OK;
}

}  // namespace aspire
