// The cross-document distance matrix of a pair's zero-padded sentence blocks, forward and backward (include/aspire_hip.h,
// aspire_sent_cdist_f32 / aspire_sent_cdist_backward_f32): what the reference's two L1 regularisers form with
//   pair_sims = -1 * torch.cdist(q_sent_reps.permute(0, 2, 1), p_sent_reps.permute(0, 2, 1))
// over the WHOLE padded block (disent_models.py:653-659 cd_l1_prop, :826-835 cd_svalue_l1_prop), and what its autograd sends back.
//
//   d_ij = ||q_i - c_j|| from the DIRECT difference for every i < q.ext, j < c.ext; a row at or beyond its document's length counts as
//   the zero vector and is never read (that is what span_mean_pool leaves there and what the reference's cdist reads): a real row
//   against a pad row gives the real row's norm, pad against pad an exact 0.
//   backward, G = dLoss / dd [P, q.ext, c.ext], through torch.cdist's rule A_ij = G_ij / d_ij, A_ij = 0 where d_ij == 0:
//     grad_q_i = sum_j A_ij (q_i - c_j)   j ascending over ALL c.ext columns (a pad column adds A_ij q_i)
//     grad_c_j = sum_i A_ij (c_j - q_i)   i ascending over ALL q.ext rows    (a pad row adds A_ij c_j)
//   pad rows of the gradients get exact zeros.
//
// Both kernels: one workgroup of four waves per pair, a lane's 12 coordinates, on pair_bwd.h's frame (PAIRED, padded sets only).
//   sent_cdist_fwd_kernel   wave w forms rows i = w, w + 4, ... of the block, one wave_sum per entry, lane 0 stores it.
//   sent_cdist_bwd_kernel   1  RE-FORMS d_ij by the forward's own loop (the same bits; nothing is kept by the forward, as in the other
//                              backward kernels) and leaves A_ij in LDS, [q.ext][c.ext] row-major: 64 KiB at 128 x 128;
//                           2  every valid row is written once, by the lanes that own its coordinates, with 16-byte stores; the
//                              differences are formed directly and weighted (not rowsum(A) q_i - sum_j A_ij c_j, which cancels).
//   No atomics, no zero fill in front: the same bits on every run.
//   poison: a document longer than its set's extent -- the forward writes NaN over the pair's whole block, the backward NaN rows
//   (the frame's rule).  A document of no rows is all pad: its partner's rows still get their gradient (their norms' derivative).
#include "pair_bwd.h"

namespace aspire {
namespace {

struct SentCdistArgs {
    RepSet q, c;
    float* dist;                // forward: [P, q.ext, c.ext]
    const float* grad_dist;     // backward: [P, q.ext, c.ext]
    float* grad_q;
    float* grad_c;
};

// sink(i, j, d_ij) for this wave's rows i = wave, wave + 4, ... < q.ext and every j < c.ext (d on every lane; pad rows are zeros)
template <class Sink>
__device__ __forceinline__ void padded_distances(const PairFrame& f, int ext_q, int ext_c, int lane, int wave, Sink&& sink) {
    const Row zero = splat(0.f);
    for (int i = wave; i < ext_q; i += kPairBwdWaves) {
        const Row x = i < f.ql ? load_row(f.qdoc + (size_t)i * kD, lane) : zero;
        for (int j = 0; j < f.cl; ++j) sink(i, j, row_length(diff(x, load_row(f.cdoc + (size_t)j * kD, lane))));
        const float norm = i < f.ql ? row_length(x) : 0.f;          // ||x - 0||: the same sum as above, formed once
        for (int j = f.cl; j < ext_c; ++j) sink(i, j, norm);
    }
}

__global__ void __launch_bounds__(kPairBwdThreads) sent_cdist_fwd_kernel(SentCdistArgs a, int rows_q, int rows_c) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t p = blockIdx.x;
    const PairFrame f = pair_frame(a.q, a.c, nullptr, nullptr, p, rows_q, rows_c);
    const int ext_q = a.q.ext, ext_c = a.c.ext;
    float* out = a.dist + (size_t)p * ext_q * ext_c;
    if (f.poison) {         // (workgroup-uniform)
        for (int e = tid; e < ext_q * ext_c; e += kPairBwdThreads) out[e] = __builtin_nanf("");
        return;
    }
    padded_distances(f, ext_q, ext_c, lane, wave, [&](int i, int j, float d) {
        if (lane == 0) out[i * ext_c + j] = d;
    });
}

__global__ void __launch_bounds__(kPairBwdThreads) sent_cdist_bwd_kernel(SentCdistArgs a, int rows_q, int rows_c) {
    extern __shared__ __attribute__((aligned(16))) float wts[];      // [ext_q][ext_c]: A_ij
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t p = blockIdx.x;
    PairFrame f = pair_frame(a.q, a.c, a.grad_q, a.grad_c, p, rows_q, rows_c);
    if (f.poison) {         // NaN rows, by the frame's writer
        skip_pair(f, lane, wave);
        return;
    }
    const int ext_q = a.q.ext, ext_c = a.c.ext, ql = f.ql, cl = f.cl;
    const float* G = a.grad_dist + (size_t)p * ext_q * ext_c;

    // ---- 1  A_ij = G_ij / d_ij over the padded block, 0 where d_ij == 0 ------------------------------------------------------------
    padded_distances(f, ext_q, ext_c, lane, wave, [&](int i, int j, float d) {
        if (lane == 0) wts[i * ext_c + j] = d > 0.f ? G[i * ext_c + j] / d : 0.f;
    });
    __syncthreads();

    // ---- 2  gradient rows ----------------------------------------------------------------------------------------------------------
    const Row zero = splat(0.f);
    for (int i = wave; i < ql; i += kPairBwdWaves) {
        const Row x = load_row(f.qdoc + (size_t)i * kD, lane);
        const float* w = wts + i * ext_c;
        Row acc = zero;
#pragma unroll 2
        for (int j = 0; j < cl; ++j) add_diff(acc, w[j], x, load_row(f.cdoc + (size_t)j * kD, lane));
        for (int j = cl; j < ext_c; ++j) add_scaled(acc, w[j], x);
        store_row(f.gq + (size_t)i * kD, lane, acc);
    }
    for (int j = wave; j < cl; j += kPairBwdWaves) {
        const Row y = load_row(f.cdoc + (size_t)j * kD, lane);
        Row acc = zero;
#pragma unroll 2
        for (int i = 0; i < ql; ++i) add_diff(acc, wts[i * ext_c + j], y, load_row(f.qdoc + (size_t)i * kD, lane));
        for (int i = ql; i < ext_q; ++i) add_scaled(acc, wts[i * ext_c + j], y);
        store_row(f.gc + (size_t)j * kD, lane, acc);
    }
    zero_pad_rows(f, lane, wave);
}

}  // namespace

// One workgroup per pair of the padded sets `q` / `c` (PAIRED: q.n == c.n; rows_q == q.ext, rows_c == c.ext).
int launch_sent_cdist(const RepSet& q, const RepSet& c, float* dist, int rows_q, int rows_c, hipStream_t stream) {
    return launch_pair_bwd(sent_cdist_fwd_kernel, SentCdistArgs{q, c, dist, nullptr, nullptr, nullptr}, c.n, 0, 0, rows_q, rows_c, stream);
}

// grad_q / grad_c are laid out like q.rows / c.rows.  LDS: the weight block, 64 KiB at the 128-row limit.
int launch_sent_cdist_backward(const RepSet& q, const RepSet& c, const float* grad_dist, float* grad_q, float* grad_c, int rows_q,
                               int rows_c, hipStream_t stream) {
    const int cap = generic_max_rows() * generic_max_rows() * (int)sizeof(float);
    const size_t lds_bytes = (size_t)rows_q * rows_c * sizeof(float);
    return launch_pair_bwd(sent_cdist_bwd_kernel, SentCdistArgs{q, c, nullptr, grad_dist, grad_q, grad_c}, c.n, lds_bytes, cap, rows_q, rows_c,
                           stream);
}

}  // namespace aspire
