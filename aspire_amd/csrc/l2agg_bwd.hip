// Backward of the three aggregations of the negated L2 block (include/aspire_hip.h, aspire_l2agg_backward_f32): the gradient of a
// pair's similarity with respect to its query and candidate sentence rows -- what the reference's autograd gives for the
// "Happens at train time" branches of allpair_masked_dist_l2max (pair_distances.py:138-186), allpair_masked_dist_l2topk (:295-345)
// and AllPairMaskedAttention.compute_distance (:95-135) under its triplet loss.
//
//   s_ij = -d_ij = -||q_i - c_j||  over the valid block (i < q_len, j < c_len);   g = dLoss / dscore of the pair;   W_ij = dscore / ds_ij
//   MAX        W = 1 at the arg-max of s, 0 elsewhere
//   TOP2       W = 1 at the two largest entries; a block of ONE entry has one pick (the reference's second pick is a masked pad
//              entry there: its gradient belongs to a pad row and is dropped)
//   ATTENTION  p = soft-max of s / temp over the block, score = sum p s:  W_ij = p_ij (1 + (s_ij - score) / temp)
//   ties: the first entry in row-major (i, j) order wins, the second pick is the next one
//   through cdist, A_ij = W_ij / d_ij and A_ij = 0 where d_ij == 0 (torch's cdist backward for coincident rows: no NaN):
//     grad_q_i = -g sum_j A_ij (q_i - c_j)        grad_c_j = +g sum_i A_ij (q_i - c_j)
//
// The frame -- one workgroup of four waves per pair, a lane's 12 coordinates, poisoned, empty and pad rows -- is pair_bwd.h's.
//   1  distances: d_ij = sqrt(sum_k (q_ik - c_jk)^2) from the DIRECT differences into LDS (row-major over the valid block), one
//      wave_sum per entry.  Nothing comes from the forward: for documents over 25 rows the forward may have used torch.cdist's
//      matmul formula (score_types.h: use_mm_formula), whose distances differ from these by rounding -- the backward's pick can
//      then differ from the forward's only where two entries are within about 3e-5 of each other, and either pick is then the
//      arg-max to that accuracy.
//   2  weights: MAX / TOP2 find their picks as the minimum of the 64-bit keys (bits of d) << 32 | (i * c_len + j) -- d >= 0, so the
//      order of the bits is the order of the values and the index breaks ties as the rule above says; ATTENTION overwrites d_ij
//      with A_ij in LDS (soft-max shifted by the block's maximum and centred as l2agg_pair.hip does: score - m = T / S).
//   3  rows: every row the pair owns is written once, by the lanes that own its coordinates, with 16-byte vector stores: the
//      differences q_i - c_j formed directly and weighted (NOT rowsum(A) q_i - sum_j A_ij c_j: that cancels when a query sentence
//      nearly equals a candidate sentence, which is where training drives them).  MAX / TOP2 touch their one or two entries.
#include "pair_bwd.h"

namespace aspire {
namespace {

constexpr int kKeyFloats = 2 * kPairBwdThreads;       // the reduction scratch in front of the distance block: 256 x 8 bytes

// minimum of the 256 threads' keys
__device__ __forceinline__ uint64_t block_min_key(uint64_t k, uint64_t* keys) {
    const int tid = threadIdx.x;
    keys[tid] = k;
    __syncthreads();
    for (int s = kPairBwdThreads / 2; s > 0; s >>= 1) {
        if (tid < s && keys[tid + s] < keys[tid]) keys[tid] = keys[tid + s];
        __syncthreads();
    }
    const uint64_t r = keys[0];
    __syncthreads();
    return r;
}
constexpr uint64_t kNoKey = ~(uint64_t)0;
__device__ __forceinline__ uint64_t key_of(float d, int e) { return ((uint64_t)__float_as_uint(d) << 32) | (uint32_t)e; }

struct L2BwdArgs {
    RepSet q, c;
    int agg;
    float temp;
    const float* grad_scores;
    float* grad_q;
    float* grad_c;
};

__global__ void __launch_bounds__(kPairBwdThreads) l2agg_bwd_kernel(L2BwdArgs a, int rows_q, int rows_c) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    uint64_t* keys = reinterpret_cast<uint64_t*>(lds);
    float* red = lds;                       // (the same scratch: a reduction finishes before the next one starts)
    float* dist = lds + kKeyFloats;         // [ql][cl]: d_ij, then (ATTENTION) A_ij
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t p = blockIdx.x;
    const PairFrame f = pair_frame(a.q, a.c, a.grad_q, a.grad_c, p, rows_q, rows_c);
    if (skip_pair(f, lane, wave)) return;
    const int ql = f.ql, cl = f.cl, n = ql * cl;
    const float *qdoc = f.qdoc, *cdoc = f.cdoc;
    float *gq = f.gq, *gc = f.gc;
    const float g = a.grad_scores[p];

    // ---- 1  distances from direct differences ---------------------------------------------------------------------------------
    direct_distances(f, dist, cl, lane, wave);
    __syncthreads();

    // ---- 2  weights -----------------------------------------------------------------------------------------------------------
    int pick_e[2] = {-1, -1};           // MAX / TOP2: the picked entries i * cl + j
    float pick_a[2] = {0.f, 0.f};       //             and their A = 1 / d (0 where d == 0)
    if (a.agg == ASPIRE_AGG_ATTENTION) {
        const float temp = a.temp;
        float m = -INFINITY;
        for (int e = tid; e < n; e += kPairBwdThreads) m = fmaxf(m, -dist[e]);
        m = block_max4(m, red);
        float S = 0.f, T = 0.f;
        for (int e = tid; e < n; e += kPairBwdThreads) {
            const float y = -dist[e] - m, w = expf(y / temp);
            S += w;
            T = fmaf(w, y, T);
        }
        S = block_sum4(S, red);
        T = block_sum4(T, red);
        const float centre = T / S;          // score - m
        for (int e = tid; e < n; e += kPairBwdThreads) {
            const float d = dist[e], y = -d - m;
            const float w = (expf(y / temp) / S) * (1.0f + (y - centre) / temp);
            dist[e] = d > 0.f ? w / d : 0.f;
        }
        __syncthreads();
    } else {
        uint64_t k = kNoKey;
        for (int e = tid; e < n; e += kPairBwdThreads) {
            const uint64_t ke = key_of(dist[e], e);
            k = ke < k ? ke : k;
        }
        const uint64_t k1 = block_min_key(k, keys);
        uint64_t k2 = kNoKey;
        if (a.agg == ASPIRE_AGG_TOP2 && n > 1) {
            k = kNoKey;
            for (int e = tid; e < n; e += kPairBwdThreads) {
                const uint64_t ke = key_of(dist[e], e);
                k = (ke != k1 && ke < k) ? ke : k;
            }
            k2 = block_min_key(k, keys);
        }
        const uint64_t ks[2] = {k1, k2};
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            if (ks[t] == kNoKey) continue;
            const float d = __uint_as_float((uint32_t)(ks[t] >> 32));
            pick_e[t] = (int)(uint32_t)ks[t];
            pick_a[t] = d > 0.f ? 1.0f / d : 0.f;
        }
    }

    // ---- 3  gradient rows -----------------------------------------------------------------------------------------------------
    const Row zero = splat(0.f);
    if (a.agg == ASPIRE_AGG_ATTENTION) {
        for (int i = wave; i < ql; i += kPairBwdWaves) {
            const Row x = load_row(qdoc + (size_t)i * kD, lane);
            Row acc = zero;
#pragma unroll 2
            for (int j = 0; j < cl; ++j) add_diff(acc, dist[i * cl + j], x, load_row(cdoc + (size_t)j * kD, lane));
            store_row(gq + (size_t)i * kD, lane, scaled(-g, acc));
        }
        for (int j = wave; j < cl; j += kPairBwdWaves) {
            const Row y = load_row(cdoc + (size_t)j * kD, lane);
            Row acc = zero;
#pragma unroll 2
            for (int i = 0; i < ql; ++i) add_diff(acc, dist[i * cl + j], load_row(qdoc + (size_t)i * kD, lane), y);
            store_row(gc + (size_t)j * kD, lane, scaled(g, acc));
        }
    } else {
        int pi[2], pj[2];
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            pi[t] = pick_e[t] < 0 ? -1 : pick_e[t] / cl;
            pj[t] = pick_e[t] < 0 ? -1 : pick_e[t] - pi[t] * cl;
        }
        for (int i = wave; i < ql; i += kPairBwdWaves) {
            Row acc = zero;
            if (i == pi[0] || i == pi[1]) {         // (wave-uniform)
                const Row x = load_row(qdoc + (size_t)i * kD, lane);
#pragma unroll
                for (int t = 0; t < 2; ++t)
                    if (i == pi[t]) add_diff(acc, pick_a[t], x, load_row(cdoc + (size_t)pj[t] * kD, lane));
                acc = scaled(-g, acc);
            }
            store_row(gq + (size_t)i * kD, lane, acc);
        }
        for (int j = wave; j < cl; j += kPairBwdWaves) {
            Row acc = zero;
            if (j == pj[0] || j == pj[1]) {
                const Row y = load_row(cdoc + (size_t)j * kD, lane);
#pragma unroll
                for (int t = 0; t < 2; ++t)
                    if (j == pj[t]) add_diff(acc, pick_a[t], load_row(qdoc + (size_t)pi[t] * kD, lane), y);
                acc = scaled(g, acc);
            }
            store_row(gc + (size_t)j * kD, lane, acc);
        }
    }
    zero_pad_rows(f, lane, wave);
}

}  // namespace

// One workgroup per pair of `q` / `c` (PAIRED: q.n == c.n); rows_q / rows_c: host-known bounds of the documents' rows
// (<= generic_max_rows()).  grad_q / grad_c are laid out like q.rows / c.rows.
int launch_l2agg_backward(const RepSet& q, const RepSet& c, int agg, float temp, const float* grad_scores, float* grad_q, float* grad_c,
                          int rows_q, int rows_c, hipStream_t stream) {
    const size_t lds_bytes = (kKeyFloats + (size_t)rows_q * rows_c) * sizeof(float);
    return launch_pair_bwd(l2agg_bwd_kernel, L2BwdArgs{q, c, agg, temp, grad_scores, grad_q, grad_c}, c.n, lds_bytes, 80 * 1024, rows_q, rows_c,
                           stream);
}

}  // namespace aspire
