// A1c: HuggingFace BertPooler, the read-out of the SimCSE baselines (src/evaluation/utils/models.py:322-357: model_out.pooler_output;
// transformers' BertPooler is nn.Linear(768, 768) on hidden_states[:, 0] followed by nn.Tanh).
//
//   pooled[b, n] = tanh( sum_k cls[b, k] * w_pool[n, k] + b_pool[n] )
//
// Both operands are K-contiguous rows: the operand form of dot_tiles.h (dotmax.hip, jointsm.hip).  Exact fp32 products on
// v_mfma_f32_16x16x4_f32, a lane holding cls[row l & 15][k] and w_pool[col l & 15][k] for k = 32 s + 8 (l >> 4) + e, the eight-k
// step mfma8 with its four accumulators -- here one set of four for the even k blocks and one for the odd ones, so a chain is 96
// terms long (the error against float64: DESIGN.md section 1).  Bias and tanhf (the library function: half of a trained pooler's
// outputs sit near +-1, where a shortcut through __expf loses the digits the cosine ranks on) in the epilogue.
//   bert_pooler_kernel  a wave forms 16 rows x 32 columns, a workgroup's four waves 16 x 128, the grid (row tiles, 6).  w_pool
//                       (2.25 MB) is read from L2; a partial last row tile reads row B - 1 again in its spare lanes and stores
//                       nothing for them.
#include <math.h>

#include "dot_tiles.h"
#include "enc_types.h"

namespace aspire {
namespace {

constexpr int kPoolWaveCols = 32, kPoolBlockCols = 4 * kPoolWaveCols;

__global__ void __launch_bounds__(256) bert_pooler_kernel(const float* __restrict__ cls, int64_t B, const float* __restrict__ w_pool,
                                                          const float* __restrict__ b_pool, float* __restrict__ pooled) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane >> 4, r = lane & 15;
    const int64_t row0 = (int64_t)blockIdx.x * 16;
    const int n0 = blockIdx.y * kPoolBlockCols + wave * kPoolWaveCols;
    const int64_t ra = row0 + r < B ? row0 + r : B - 1;                 // spare lanes of the last tile: a row that exists
    const float* pa = cls + ra * kD + 8 * g;
    const float* pb = w_pool + (int64_t)(n0 + r) * kD + 8 * g;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    f32x4 acc[2][2][4];                                                 // [k block parity][column tile][mfma8's four]
#pragma unroll
    for (int i = 0; i < 16; ++i) (&acc[0][0][0])[i] = zero;
#pragma unroll 2
    for (int s = 0; s < kD / 32; s += 2) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int k = 32 * (s + h);
            const f32x4 a0 = ld4(pa + k), a1 = ld4(pa + k + 4);
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                const f32x4 b0 = ld4(pb + t * 16 * kD + k), b1 = ld4(pb + t * 16 * kD + k + 4);
                mfma8(a0, a1, b0, b1, acc[h][t]);
            }
        }
    }
    // C[row 4 g + v][col r]: cls row row0 + 4 g + v, output column n0 + 16 t + r
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const f32x4 dot = ((acc[0][t][0] + acc[0][t][1]) + (acc[0][t][2] + acc[0][t][3])) +
                          ((acc[1][t][0] + acc[1][t][1]) + (acc[1][t][2] + acc[1][t][3]));
        const int n = n0 + 16 * t + r;
        const float bias = b_pool[n];
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            const int64_t row = row0 + 4 * g + v;
            if (row < B) pooled[row * kD + n] = tanhf(dot[v] + bias);
        }
    }
}

}  // namespace

int launch_pooler(const float* cls, int64_t B, const float* w_pool, const float* b_pool, float* pooled, hipStream_t st) {
    static_assert(kD % kPoolBlockCols == 0 && kD % 64 == 0, "whole column blocks, an even count of k blocks");
    const int64_t row_tiles = (B + 15) / 16;
    ASPIRE_REQUIRE(row_tiles < ((int64_t)1 << 31), ASPIRE_ERR_UNSUPPORTED, "too many rows for one pooler launch: %lld", (long long)B);
    hipLaunchKernelGGL(bert_pooler_kernel, dim3((unsigned)row_tiles, kD / kPoolBlockCols), dim3(256), 0, st, cls, B, w_pool, b_pool, pooled);
    ASPIRE_LAUNCH_OK();
    return ASPIRE_OK;
}

}  // namespace aspire
