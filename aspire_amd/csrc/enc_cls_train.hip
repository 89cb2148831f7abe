// The kernels that train the CLS-row models (encoder_bwd.hip is the host side: aspire_bert_cls_mix_train_f32,
// aspire_bert_layers_backward_cls_f32, aspire_inbatch_xent_f32 / _backward_f32).
//
// Kernels
//   cls_mix_tap_kernel        the CLS row of every hidden state of a training forward (the tape's layer inputs and hidden_out) ->
//                             layer_cls [n_layers + 1, B, 768] and their mix sum_l mix[l] state_l[b, 0, :], l ascending -- MySPECTER's
//                             doc_reps_bert (disent_models.py:178-205) behind the encoder call; without a mix the top state's rows,
//                             copied                                                     (one wave per document, four per workgroup)
//   cls_inject_kernel         row (b, 0) of a [B, L, 768] gradient += f grad_cls[b, :], f = mix[l] or 1: the read-out's gradient
//                             source, B rows                                                               (one wave per document)
//   cls_grad_mix_kernel       grad_mix[l] = sum_b <grad_cls[b], layer_cls[l, b]> in double, rounded once: a thread's chain runs over its
//                             coordinates of the documents b = wave, wave + 4, ..., then one fixed tree     (one workgroup per l)
//   xent_row_block (device)   ICTBERTWrapper.forward_rank's s = Q C^T (sentsim_models.py:81-126) over B <= 128 rows, sixteen rows at a
//                             time: wave w the 16 x 16 tile of columns 16 w on dot_tiles.h's operand and product steps
//                             (v_mfma_f32_16x16x4_f32: exact fp32 products, sixteen accumulators), the tiles meet in LDS and a wave
//                             forms two rows' maximum m and z = sum exp(s - m).  m and z stay apart: CLS rows of one model give |s|
//                             of several hundred, where one ulp (6e-5) is as large as log z of a confident row
//   inbatch_xent_kernel       row_lse[i] = m_i + log z_i and loss = sum_i ((m_i - s_ii) + log z_i), the B terms in one fixed tree:
//                             one workgroup of eight waves walks the row blocks                                  (one launch)
//   inbatch_xent_bwd_kernel   W_ij = grad_loss (exp(s_ij - m_i) / z_i - [i == j]); a workgroup owns 16 rows of grad_q (grad_q[i] =
//                             sum_j W_ij c_j: its own row block) or of grad_c (grad_c[j] = sum_i W_ij q_i: its 16 columns of every
//                             row block, each with that block's m and z), keeps W in LDS and writes each of its rows once with
//                             16-byte stores.  Nothing is read from the forward.  Two forms that were tried first missed the float64
//                             test on two towers' CLS rows (|s| about 700): direct FMA dot products against the forward's row_lse
//                             (jointsm_bwd.hip's form) left the rows of W summing to 1e-4 instead of 0, and that much of the towers'
//                             common direction leaked into every gradient (ten times the bound); the forward's own products
//                             against row_lse left 5 ulp in the top LayerNorm bias's gradient (1.3 times the bound), the rounding
//                             of m + log z to one float
// No atomics: every element has one writer and every sum a fixed order, so two runs give the same bits.
#include <math.h>

#include "enc_types.h"
#include "dot_tiles.h"
#include "pair_bwd.h"

namespace aspire {
namespace {

constexpr int kTapDocs = 4;                 // documents per workgroup of the tap and inject kernels (one per wave)
constexpr int kXentTile = 16;               // rows of s in a row block
constexpr int kXentThreads = 512;           // eight waves, one per 16-column tile of B <= 128
constexpr int kSStride = kXentMaxRows + 4;  // LDS row stride of a row block of s (kXStride's padding)

// the first packed row of document b (clamped into the packed rows: the lists are the caller's device memory)
__device__ __forceinline__ int64_t first_packed_row(const ClsRows& p, int64_t b) { return min(max(p.doc_start[b], 0), p.rows - 1); }

// packed (p.doc_start not NULL): the tape's states are [rows, 768] and the CLS row is the document's first packed row; the top state is
// the padded hidden_out, where that row is row_src[first packed row]
__device__ __forceinline__ const float* cls_row(const ClsStates& s, int l, int64_t b, int64_t L, const ClsRows& p) {
    const float* base = l < s.n_layers ? reinterpret_cast<const float*>(s.x0 + (size_t)l * s.layer_stride) : s.top;
    if (p.doc_start) {
        const int64_t m = first_packed_row(p, b);
        return base + (size_t)(l < s.n_layers ? m : min(max(p.row_src[m], 0), p.padded_rows - 1)) * kD;
    }
    return base + (size_t)b * L * kD;
}

__global__ void __launch_bounds__(64 * kTapDocs) cls_mix_tap_kernel(ClsStates s, int64_t B, int64_t L, const float* __restrict__ mix,
                                                                    float* __restrict__ cls_out, float* __restrict__ layer_cls, ClsRows p) {
    const int lane = threadIdx.x & 63;
    const int64_t b = (int64_t)blockIdx.x * kTapDocs + (threadIdx.x >> 6);
    if (b >= B) return;
    Row acc = splat(0.f);
    for (int l = (mix || layer_cls) ? 0 : s.n_layers; l <= s.n_layers; ++l) {
        const Row v = load_row(cls_row(s, l, b, L, p), lane);
        if (layer_cls) store_row(layer_cls + ((size_t)l * B + b) * kD, lane, v);
        if (mix) {
            const Row t = scaled(mix[l], v);
            acc = l == 0 ? t : Row{acc.x + t.x, acc.y + t.y, acc.z + t.z};
        } else if (l == s.n_layers) {
            acc = v;
        }
    }
    store_row(cls_out + (size_t)b * kD, lane, acc);
}

__global__ void __launch_bounds__(64 * kTapDocs) cls_inject_kernel(float* __restrict__ grad, int64_t B, int64_t L,
                                                                   const float* __restrict__ grad_cls, const float* __restrict__ mix, int l,
                                                                   ClsRows p) {
    const int lane = threadIdx.x & 63;
    const int64_t b = (int64_t)blockIdx.x * kTapDocs + (threadIdx.x >> 6);
    if (b >= B) return;
    float* row = grad + (size_t)(p.doc_start ? first_packed_row(p, b) : b * L) * kD;     // (packed: a [rows, 768] gradient)
    Row d = load_row(row, lane);
    add_scaled(d, mix ? mix[l] : 1.0f, load_row(grad_cls + (size_t)b * kD, lane));
    store_row(row, lane, d);
}

__global__ void __launch_bounds__(kPairBwdThreads) cls_grad_mix_kernel(const float* __restrict__ grad_cls, const float* __restrict__ layer_cls,
                                                                       int64_t B, float* __restrict__ grad_mix) {
    __shared__ double red[kPairBwdThreads];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float* rows = layer_cls + (size_t)blockIdx.x * B * kD;
    // in double: the soft-max backward behind this sum takes differences of its n_layers + 1 results (the states' CLS rows resemble each
    // other), so one fp32 rounding of each result is all the error the sum may bring -- B x 768 double FMAs per state cost nothing
    double acc = 0.0;
    for (int64_t b = wave; b < B; b += kPairBwdWaves) {
        const Row g = load_row(grad_cls + (size_t)b * kD, lane), y = load_row(rows + (size_t)b * kD, lane);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            acc = fma((double)g.x[e], (double)y.x[e], acc);
            acc = fma((double)g.y[e], (double)y.y[e], acc);
            acc = fma((double)g.z[e], (double)y.z[e], acc);
        }
    }
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int half = kPairBwdThreads / 2; half > 0; half >>= 1) {        // one fixed tree
        if ((int)threadIdx.x < half) red[threadIdx.x] += red[threadIdx.x + half];
        __syncthreads();
    }
    if (threadIdx.x == 0) grad_mix[blockIdx.x] = (float)red[0];
}

// the 16 x 16 tile s[i0 + 4 g + v][j0 + r] (g = lane >> 4, r = lane & 15) in element v; rows at or beyond B enter as zeros
__device__ __forceinline__ f32x4 xent_tile(const float* __restrict__ q, const float* __restrict__ c, int i0, int j0, int B, int lane) {
    const int r = lane & 15, g = lane >> 4;
    const bool va = i0 + r < B, vb = j0 + r < B;
    const float* pa = q + (size_t)(va ? i0 + r : 0) * kD + 8 * g;
    const float* pb = c + (size_t)(vb ? j0 + r : 0) * kD + 8 * g;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    // sixteen accumulators, as jointsm.hip spreads its k blocks (set u: blocks s = u mod 4): chains of 12 products, not 48 -- CLS rows
    // of one model give s of several hundred with differences of a few units, and the soft-max sees only the differences
    f32x4 acc[4][4];
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[u][e] = zero;
#pragma unroll
    for (int s = 0; s < kD / 32; ++s) {
        const f32x4 a0 = va ? ld4(pa + 32 * s) : zero, a1 = va ? ld4(pa + 32 * s + 4) : zero;
        const f32x4 b0 = vb ? ld4(pb + 32 * s) : zero, b1 = vb ? ld4(pb + 32 * s + 4) : zero;
        mfma8(a0, a1, b0, b1, acc[s & 3]);
    }
    return tile_dots(acc);
}

// Rows 16 it .. 16 it + 15 of s against all B columns into S (wave w the tile of columns 16 w), then every row's maximum m and
// z = sum_j exp(s_ij - m) into stat[row] and stat[16 + row].  All eight waves call; the block is published on return.  Kept apart, m
// and z carry what m + log z loses at |s| of several hundred (one ulp of 700 is 6e-5: as large as log z of a confident row).
__device__ __forceinline__ void xent_row_block(const float* __restrict__ q, const float* __restrict__ c, int it, int B, float* S, float* stat,
                                               int lane, int wave) {
    const int r = lane & 15, g = lane >> 4, i0 = it * kXentTile, j0 = wave * kXentTile;
    if (j0 < B) {        // (wave-uniform)
        const f32x4 d = xent_tile(q, c, i0, j0, B, lane);
#pragma unroll
        for (int v = 0; v < 4; ++v) S[(4 * g + v) * kSStride + j0 + r] = d[v];
    }
    __syncthreads();
#pragma unroll
    for (int rr = 0; rr < 2; ++rr) {        // (rows at or beyond B hold the products of zero rows: finite, never used)
        const int row = 2 * wave + rr;
        const float x0 = lane < B ? S[row * kSStride + lane] : -INFINITY;
        const float x1 = lane + 64 < B ? S[row * kSStride + lane + 64] : -INFINITY;
        const float m = wave_max(fmaxf(x0, x1));
        const float z = wave_sum((lane < B ? expf(x0 - m) : 0.f) + (lane + 64 < B ? expf(x1 - m) : 0.f));
        if (lane == 0) {
            stat[row] = m;
            stat[kXentTile + row] = z;
        }
    }
    __syncthreads();
}

// one workgroup walks the row blocks: row_lse[i] = m_i + log z_i, and the loss from (m_i - s_ii) + log z_i, the B terms in one tree
__global__ void __launch_bounds__(kXentThreads) inbatch_xent_kernel(const float* __restrict__ q, const float* __restrict__ c, int B,
                                                                    float* __restrict__ loss, float* __restrict__ row_lse) {
    __shared__ float S[kXentTile * kSStride];
    __shared__ float stat[2 * kXentTile];
    __shared__ float term[kXentMaxRows];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid < kXentMaxRows) term[tid] = 0.f;
    for (int it = 0; it * kXentTile < B; ++it) {
        xent_row_block(q, c, it, B, S, stat, lane, wave);
        const int i = it * kXentTile + tid;
        if (tid < kXentTile && i < B) {
            const float m = stat[tid], lz = logf(stat[kXentTile + tid]);
            row_lse[i] = m + lz;
            term[i] = (m - S[tid * kSStride + i]) + lz;
        }
        __syncthreads();        // S and stat are written again
    }
    __syncthreads();
    if (wave == 0) {
        const float t = wave_sum(term[lane] + term[lane + 64]);
        if (lane == 0) loss[0] = t;
    }
}

// blockIdx.y 0: the workgroup owns 16 rows of grad_q (other = c) and needs its own row block of s; 1: 16 rows of grad_c (other = q) and
// needs its 16 columns of EVERY row with that row's m and z, so it walks all row blocks.  W_ij = gl (exp(s_ij - m_i) / z_i - [i == j]).
__global__ void __launch_bounds__(kXentThreads) inbatch_xent_bwd_kernel(const float* __restrict__ q, const float* __restrict__ c, int B,
                                                                        const float* __restrict__ grad_loss, float* __restrict__ grad_q,
                                                                        float* __restrict__ grad_c) {
    __shared__ float S[kXentTile * kSStride];           // a row block of s; for grad_q then W [own row][j]
    __shared__ float Wc[kXentTile * kSStride];          // for grad_c: W [own column][i]
    __shared__ float stat[2 * kXentTile];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const bool cside = blockIdx.y != 0;
    const float* other = cside ? q : c;
    float* out = cside ? grad_c : grad_q;
    const int o0 = blockIdx.x * kXentTile;
    const int no = B - o0 < kXentTile ? B - o0 : kXentTile;
    const float gl = grad_loss[0];
    // 1  the weights
    const int first = cside ? 0 : (int)blockIdx.x, last = cside ? (B + kXentTile - 1) / kXentTile : (int)blockIdx.x + 1;
    for (int it = first; it < last; ++it) {
        xent_row_block(q, c, it, B, S, stat, lane, wave);
        if (!cside) {
            for (int e = tid; e < kXentTile * B; e += kXentThreads) {
                const int row = e / B, j = e - row * B;
                float* w = S + row * kSStride + j;
                *w = gl * (expf(*w - stat[row]) / stat[kXentTile + row] - (o0 + row == j ? 1.0f : 0.0f));
            }
        } else if (tid < kXentTile * kXentTile) {
            const int row = tid >> 4, jl = tid & 15, i = it * kXentTile + row, j = o0 + jl;
            Wc[jl * kSStride + i] =
                i < B && j < B ? gl * (expf(S[row * kSStride + j] - stat[row]) / stat[kXentTile + row] - (i == j ? 1.0f : 0.0f)) : 0.f;
        }
        __syncthreads();
    }
    // 2  the rows
    const float* W = cside ? Wc : S;
    for (int o = wave; o < no; o += kXentThreads / 64) {
        Row acc = splat(0.f);
#pragma unroll 2
        for (int k = 0; k < B; ++k) add_scaled(acc, W[o * kSStride + k], load_row(other + (size_t)k * kD, lane));
        store_row(out + (size_t)(o0 + o) * kD, lane, acc);
    }
}

}  // namespace

int launch_cls_mix_tap(const ClsStates& s, int64_t B, int64_t L, const float* mix, float* cls_out, float* layer_cls, hipStream_t st,
                       const ClsRows* packed) {
    hipLaunchKernelGGL(cls_mix_tap_kernel, dim3((unsigned)((B + kTapDocs - 1) / kTapDocs)), dim3(64 * kTapDocs), 0, st, s, B, L, mix, cls_out,
                       layer_cls, packed ? *packed : ClsRows{});
    ASPIRE_LAUNCH_OK();
    return ASPIRE_OK;
}

int launch_cls_inject(float* grad, int64_t B, int64_t L, const float* grad_cls, const float* mix, int l, hipStream_t st, const ClsRows* packed) {
    hipLaunchKernelGGL(cls_inject_kernel, dim3((unsigned)((B + kTapDocs - 1) / kTapDocs)), dim3(64 * kTapDocs), 0, st, grad, B, L, grad_cls, mix,
                       l, packed ? *packed : ClsRows{});
    ASPIRE_LAUNCH_OK();
    return ASPIRE_OK;
}

int launch_cls_grad_mix(const float* grad_cls, const float* layer_cls, int64_t B, int n_states, float* grad_mix, hipStream_t st) {
    hipLaunchKernelGGL(cls_grad_mix_kernel, dim3((unsigned)n_states), dim3(kPairBwdThreads), 0, st, grad_cls, layer_cls, B, grad_mix);
    ASPIRE_LAUNCH_OK();
    return ASPIRE_OK;
}

int launch_inbatch_xent(const float* q, const float* c, int B, float* loss, float* row_lse, hipStream_t st) {
    hipLaunchKernelGGL(inbatch_xent_kernel, dim3(1), dim3(kXentThreads), 0, st, q, c, B, loss, row_lse);
    ASPIRE_LAUNCH_OK();
    return ASPIRE_OK;
}

int launch_inbatch_xent_backward(const float* q, const float* c, int B, const float* grad_loss, float* grad_q, float* grad_c, hipStream_t st) {
    hipLaunchKernelGGL(inbatch_xent_bwd_kernel, dim3((unsigned)((B + kXentTile - 1) / kXentTile), 2), dim3(kXentThreads), 0, st, q, c, B,
                       grad_loss, grad_q, grad_c);
    ASPIRE_LAUNCH_OK();
    return ASPIRE_OK;
}

}  // namespace aspire
