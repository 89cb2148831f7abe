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
// The frame -- one workgroup of four waves per pair, a lane's 12 coordinates, poisoned, empty and pad rows -- is pair_bwd.h's.
//   1  products: d_ij into LDS (row-major over the valid block) as DIRECT fp32 FMA dot products, one wave_sum per entry -- the form
//      in which pair_bwd.h makes the L2 distances, not dot_tiles.h's matrix products: a lane's chain is 12 fmaf long and the rest a
//      balanced tree over the 64 lanes, which rounds less than the forward's 48-long chains, and the block is formed once.  Nothing
//      comes from the forward.
//   2  weights: the block's maximum, Z and T with the four waves' partial results combined in one fixed order, then d_ij is
//      overwritten with W_ij in place.
//   3  rows: every row the pair owns is written once, by the lanes that own its coordinates, with 16-byte vector stores: sum_j W_ij c_j
//      (sum_i W_ij q_i) accumulated in registers in index order and scaled by g.
#include "pair_bwd.h"

namespace aspire {
namespace {

constexpr int kRedFloats = 16;          // the reduction scratch in front of the product block (four floats used; 64 bytes keep the block aligned)

struct JsmBwdArgs {
    RepSet q, c;
    const float* grad_scores;
    float* grad_q;
    float* grad_c;
};

__global__ void __launch_bounds__(kPairBwdThreads) jointsm_bwd_kernel(JsmBwdArgs a, int rows_q, int rows_c) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float* red = lds;
    float* dots = lds + kRedFloats;         // [ql][cl]: d_ij, then W_ij
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t p = blockIdx.x;
    const PairFrame f = pair_frame(a.q, a.c, a.grad_q, a.grad_c, p, rows_q, rows_c);
    if (skip_pair(f, lane, wave)) return;
    const int ql = f.ql, cl = f.cl, n = ql * cl;
    const float *qdoc = f.qdoc, *cdoc = f.cdoc;
    float *gq = f.gq, *gc = f.gc;
    const float g = a.grad_scores[p];

    // ---- 1  dot products ------------------------------------------------------------------------------------------------------
    for (int i = wave; i < ql; i += kPairBwdWaves) {
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
    for (int e = tid; e < n; e += kPairBwdThreads) m = fmaxf(m, dots[e]);
    m = block_max4(m, red);
    float Z = 0.f, T = 0.f;
    for (int e = tid; e < n; e += kPairBwdThreads) {
        const float y = dots[e] - m, w = expf(y / root);
        Z += w;
        T = fmaf(w, y, T);
    }
    Z = block_sum4(Z, red);
    T = block_sum4(T, red);
    const float centre = T / Z;          // E - m
    for (int e = tid; e < n; e += kPairBwdThreads) {
        const float y = dots[e] - m;
        dots[e] = 2.0f * (expf(y / root) / Z) * (1.0f + (y - centre) / root);
    }
    __syncthreads();

    // ---- 3  gradient rows -----------------------------------------------------------------------------------------------------
    const Row zero = splat(0.f);
    for (int i = wave; i < ql; i += kPairBwdWaves) {
        Row acc = zero;
#pragma unroll 2
        for (int j = 0; j < cl; ++j) add_scaled(acc, dots[i * cl + j], load_row(cdoc + (size_t)j * kD, lane));
        store_row(gq + (size_t)i * kD, lane, scaled(g, acc));
    }
    for (int j = wave; j < cl; j += kPairBwdWaves) {
        Row acc = zero;
#pragma unroll 2
        for (int i = 0; i < ql; ++i) add_scaled(acc, dots[i * cl + j], load_row(qdoc + (size_t)i * kD, lane));
        store_row(gc + (size_t)j * kD, lane, scaled(g, acc));
    }
    zero_pad_rows(f, lane, wave);
}

}  // namespace

// One workgroup per pair of `q` / `c` (PAIRED: q.n == c.n); rows_q / rows_c: host-known bounds of the documents' rows
// (<= generic_max_rows()).  grad_q / grad_c are laid out like q.rows / c.rows.
int launch_jointsm_backward(const RepSet& q, const RepSet& c, const float* grad_scores, float* grad_q, float* grad_c, int rows_q,
                            int rows_c, hipStream_t stream) {
    const size_t lds_bytes = (kRedFloats + (size_t)rows_q * rows_c) * sizeof(float);
    return launch_pair_bwd(jointsm_bwd_kernel, JsmBwdArgs{q, c, grad_scores, grad_q, grad_c}, c.n, lds_bytes, 80 * 1024, rows_q, rows_c, stream);
}

}  // namespace aspire
