// Backward of the joint soft-max alignment score (include/aspire_hip.h, aspire_jointsm_backward_f32): the gradient of a pair's
// similarity S = 2 sum_ij p_ij d_ij with respect to its query and candidate sentence rows -- what the reference's autograd gives for
// allpair_joint_sm_negscore (pair_distances.py:348-402) through torch.bmm, masked_2d_softmax (activations.py:35-61) and the two
// alignment loops, the dist_function of WordSentAlignPolyEnc's triplet loss (disent_models.py:868-875).
//
//   d_ij = <q_i, c_j> over the valid block (i < q_len, j < c_len);  p = soft-max of d / sqrtf(768) over the block jointly
//   g = dLoss / dS of the pair;   E = sum p d;   W_ij = dS / dd_ij = 2 p_ij (1 + (d_ij - E) / sqrtf(768))
//   grad_q_i = g sum_j W_ij c_j        grad_c_j = g sum_i W_ij q_i
//   shifted by the block's maximum m, as l2agg_pair.hip centres its attention (d reaches about 1000 on rows of norm 28: d - E must
//   not cancel against a large E):
//     e_ij = exp((d_ij - m) / sqrtf(768)),  Z = sum e,  T = sum e (d_ij - m),  E - m = T / Z
//     W_ij = 2 (e_ij / Z) (1 + ((d_ij - m) - T / Z) / sqrtf(768))
//
// l2agg_bwd.hip's frame: one workgroup of four waves per pair (ASPIRE_PAIR_PAIRED: every document belongs to one pair, so a gradient
// row has one writer -- no atomics, nothing summed across workgroups, the same bits on every run).  A lane owns 12 of the 768
// coordinates (three 16-byte pieces), a wave the rows r = wave, wave + 4, ...
//   1  products: d_ij into LDS (row-major over the valid block) as DIRECT fp32 FMA dot products, one wave_sum per entry -- the form
//      in which l2agg_bwd.hip makes its distances, not dot_tiles.h's matrix products: a lane's chain is 12 fmaf long and the rest a
//      balanced tree over the 64 lanes, which rounds less than the forward's 48-long chains, and the block is formed once.  Nothing
//      comes from the forward.
//   2  weights: the block's maximum, Z and T with the four waves' partial results combined in one fixed order, then d_ij is
//      overwritten with W_ij in place.
//   3  rows: every row the pair owns is written once, by the lanes that own its coordinates, with 16-byte vector stores: sum_j W_ij c_j
//      (sum_i W_ij q_i) accumulated in registers in index order and scaled by g; pad rows of padded sets (len <= r < ext) get exact
//      zeros.
// A document longer than its set's host-known bound has its rows (up to the bound) set to NaN, as the forward poisons its score.
#include <math.h>

#include "common.h"
#include "score_types.h"

namespace aspire {
namespace {

constexpr int kJbThreads = 256, kJbWaves = kJbThreads / 64;
constexpr int kRedFloats = 16;          // the reduction scratch in front of the product block (four floats used; 64 bytes keep the block aligned)

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
// acc += w a
__device__ __forceinline__ void add_scaled(Row& acc, float w, const Row& a) {
    const v4 ww = {w, w, w, w};
    acc.x = __builtin_elementwise_fma(ww, a.x, acc.x);
    acc.y = __builtin_elementwise_fma(ww, a.y, acc.y);
    acc.z = __builtin_elementwise_fma(ww, a.z, acc.z);
}
__device__ __forceinline__ Row scaled(float f, const Row& r) { return Row{f * r.x, f * r.y, f * r.z}; }

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

struct JsmBwdArgs {
    RepSet q, c;
    const float* grad_scores;
    float* grad_q;
    float* grad_c;
};

__global__ void __launch_bounds__(kJbThreads) jointsm_bwd_kernel(JsmBwdArgs a, int rows_q, int rows_c) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float* red = lds;
    float* dots = lds + kRedFloats;         // [ql][cl]: d_ij, then W_ij
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t p = blockIdx.x;
    const int q_len = a.q.len[p], c_len = a.c.len[p];
    const bool poison = q_len > rows_q || c_len > rows_c;              // longer than the host-known bound
    const int ql = q_len < 0 ? 0 : (q_len > rows_q ? rows_q : q_len), cl = c_len < 0 ? 0 : (c_len > rows_c ? rows_c : c_len);
    const int q_own = a.q.ext > 0 ? a.q.ext : ql, c_own = a.c.ext > 0 ? a.c.ext : cl;        // rows this pair writes (pad rows included)
    const float* qdoc = a.q.rows + (size_t)a.q.start[p] * kD;
    const float* cdoc = a.c.rows + (size_t)a.c.start[p] * kD;
    float* gq = a.grad_q + (size_t)a.q.start[p] * kD;
    float* gc = a.grad_c + (size_t)a.c.start[p] * kD;
    const int n = ql * cl;
    if (poison || n == 0) {             // (workgroup-uniform)
        const float v = poison ? __builtin_nanf("") : 0.f;
        for (int r = wave; r < q_own; r += kJbWaves) store_row(gq + (size_t)r * kD, lane, splat(r < ql ? v : 0.f));
        for (int r = wave; r < c_own; r += kJbWaves) store_row(gc + (size_t)r * kD, lane, splat(r < cl ? v : 0.f));
        return;
    }
    const float g = a.grad_scores[p];

    // ---- 1  dot products ------------------------------------------------------------------------------------------------------
    for (int i = wave; i < ql; i += kJbWaves) {
        const Row x = load_row(qdoc + (size_t)i * kD, lane);
        for (int j = 0; j < cl; ++j) {
            const Row y = load_row(cdoc + (size_t)j * kD, lane);
            const v4 s = __builtin_elementwise_fma(x.z, y.z, __builtin_elementwise_fma(x.y, y.y, x.x * y.x));
            const float d = wave_sum((s.x + s.y) + (s.z + s.w));
            if (lane == 0) dots[i * cl + j] = d;
        }
    }
    __syncthreads();

    // ---- 2  weights -----------------------------------------------------------------------------------------------------------
    const float root = sqrtf((float)kD);
    float m = -INFINITY;
    for (int e = tid; e < n; e += kJbThreads) m = fmaxf(m, dots[e]);
    m = block_max4(m, red);
    float Z = 0.f, T = 0.f;
    for (int e = tid; e < n; e += kJbThreads) {
        const float y = dots[e] - m, w = expf(y / root);
        Z += w;
        T = fmaf(w, y, T);
    }
    Z = block_sum4(Z, red);
    T = block_sum4(T, red);
    const float centre = T / Z;          // E - m
    for (int e = tid; e < n; e += kJbThreads) {
        const float y = dots[e] - m;
        dots[e] = 2.0f * (expf(y / root) / Z) * (1.0f + (y - centre) / root);
    }
    __syncthreads();

    // ---- 3  gradient rows -----------------------------------------------------------------------------------------------------
    const Row zero = splat(0.f);
    for (int i = wave; i < ql; i += kJbWaves) {
        Row acc = zero;
#pragma unroll 2
        for (int j = 0; j < cl; ++j) add_scaled(acc, dots[i * cl + j], load_row(cdoc + (size_t)j * kD, lane));
        store_row(gq + (size_t)i * kD, lane, scaled(g, acc));
    }
    for (int j = wave; j < cl; j += kJbWaves) {
        Row acc = zero;
#pragma unroll 2
        for (int i = 0; i < ql; ++i) add_scaled(acc, dots[i * cl + j], load_row(qdoc + (size_t)i * kD, lane));
        store_row(gc + (size_t)j * kD, lane, scaled(g, acc));
    }
    for (int r = ql + wave; r < q_own; r += kJbWaves) store_row(gq + (size_t)r * kD, lane, zero);
    for (int r = cl + wave; r < c_own; r += kJbWaves) store_row(gc + (size_t)r * kD, lane, zero);
}

}  // namespace

// One workgroup per pair of `q` / `c` (PAIRED: q.n == c.n); rows_q / rows_c: host-known bounds of the documents' rows
// (<= generic_max_rows()).  grad_q / grad_c are laid out like q.rows / c.rows.
int launch_jointsm_backward(const RepSet& q, const RepSet& c, const float* grad_scores, float* grad_q, float* grad_c, int rows_q,
                            int rows_c, hipStream_t stream) {
    ASPIRE_REQUIRE(rows_q <= generic_max_rows() && rows_c <= generic_max_rows(), ASPIRE_ERR_UNSUPPORTED,
                   "documents with more than %d sentence rows are not supported (got %d x %d)", generic_max_rows(), rows_q, rows_c);
    const int64_t P = c.n;
    if (P == 0) return ASPIRE_OK;
    ASPIRE_REQUIRE(P < ((int64_t)1 << 31), ASPIRE_ERR_UNSUPPORTED, "too many pairs: %lld", (long long)P);
    const size_t lds_bytes = (size_t)(kRedFloats + rows_q * rows_c) * sizeof(float);
    if (lds_bytes > 64 * 1024) {      // more than the default dynamic LDS limit: raise it (per function, sticky, harmless to repeat)
        ASPIRE_HIP_OK(hipFuncSetAttribute(reinterpret_cast<const void*>(jointsm_bwd_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                          80 * 1024));
    }
    JsmBwdArgs a{q, c, grad_scores, grad_q, grad_c};
    hipLaunchKernelGGL(jointsm_bwd_kernel, dim3((unsigned)P), dim3(kJbThreads), lds_bytes, stream, a, rows_q, rows_c);
    ASPIRE_LAUNCH_OK();
    return ASPIRE_OK;
}

}  // namespace aspire
