// A1: the BERT-base encoder forward that AspireConSent runs before pooling
// (examples/ex_aspire_consent.py:72-73: self.bert_encoder(tokid_tt, token_type_ids=seg_tt,
// attention_mask=attnmask_tt).last_hidden_state; the arithmetic itself is HuggingFace transformers'
// BertModel, pinned 4.5.1 in the reference's requirements.txt:14).
//
// Precision: the north star asks for sentence reps within 1e-4 of the fp32 CPU path through 12 layers: every GEMM is
// fp32-accurate.  The nn.Linear GEMMs (95 % of the flops) run on the bf16 matrix pipe with every fp32 operand split into
// three bf16 planes and six products per term (gemm_bf16x3_kernel: same error against float64 as the fp32-input MFMA,
// 1.4-1.6x its speed); attention (flash_attn_f32_kernel) and the A/B form (ASPIRE_HIP_GEMM=f32) use the fp32-input matrix
// cores (v_mfma_f32_32x32x2_f32: exact fp32 FMA chains, 157 TFLOP/s peak on MI355X -- still the figure the encoder's
// throughput is quoted against, so the bf16x3 form can exceed 100 % of it).  Plain bf16 inputs give ~1e-2: not an option.
//
// Kernels
//   embed_layernorm_kernel   word + position + token-type gather, LayerNorm          (one wave per token)
//   gemm_bf16x3_kernel       C = A.B^T (+bias)(+GELU)(+residual) for nn.Linear shapes (see above)
//   gemm_f32_kernel          C = alpha * A.B^T (+bias)(+GELU)(+residual), batched/strided; A [M,K] k-contiguous,
//                            B either [N,K] k-contiguous (nn.Linear weight, K^T of attention) or [K,N]
//                            n-contiguous (V of attention).  128x128 / 128x64 / 64x64 block tiles, BK = 16,
//                            4 waves as 2x2, LDS tiles stored k-major so MFMA operand reads are
//                            conflict-free ds_read_b32, register-staged double buffering.
//   softmax_mask_kernel      rows of scores: x*scale + key-padding bias, softmax in place (one wave per row)
//   layernorm_kernel         y = LN(x) * gamma + beta, eps 1e-12                       (one wave per token)
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include "common.h"
#include "tuning.h"

namespace aspire {
namespace {

using f32x16 = __attribute__((ext_vector_type(16))) float;

struct GemmArgs {
    const float* A;     // [batch][M][lda]
    const float* B;     // B_KN ? [batch][K][ldb] : [batch][N][ldb]
    float* C;           // [batch][M][ldc]
    const float* bias;  // [N] or null
    const float* res;   // [M][ldr] residual or null (not batched)
    int M, N, K;
    int lda, ldb, ldc, ldr;
    // batch index z = z1 * nz2 + z2; operand offsets are z1 * s?1 + z2 * s?2 (attention: z1 = doc, z2 = head)
    int nz2;
    long long sa1, sa2, sb1, sb2, sc1, sc2;
    float alpha;
    int gelu;
};

// GELU as HF BertModel's "gelu" (0.5 x (1 + erf(x / sqrt 2))), written around erfc: e = erfc(|x| / sqrt 2) = 2^q(|x|), q a degree-8 polynomial
// (a weighted Chebyshev fit of log2 erfc(t / sqrt 2) on [0, 5.8]; beyond, erfc < 7e-9), then x - 0.5 x e for x > 0 and 0.5 x e otherwise: no
// cancellation on either side, 15 VALU instructions where 0.5 x (1 + erff(.)) takes 37 (50 M activations per FFN1 launch at 64 x 256 tokens).
// Max |error| against float64 over [-9, 9]: 2.5e-7 (the erff form, rounded in fp32: 4.5e-7).
__device__ __forceinline__ float gelu_erf(float x) {
    const float t = fminf(fabsf(x), 5.8f);
    float q = -1.9605818124546204e-06f;
    q = fmaf(q, t, 2.8825294066336937e-05f);
    q = fmaf(q, t, -0.0001355033746222034f);
    q = fmaf(q, t, -0.0002612900862004608f);
    q = fmaf(q, t, 0.007229907438158989f);
    q = fmaf(q, t, -0.05261624604463577f);
    q = fmaf(q, t, -0.4591653645038605f);
    q = fmaf(q, t, -1.1511112451553345f);
    q = fmaf(q, t, 1.7379414884999278e-07f);
    const float r = 0.5f * x * __builtin_amdgcn_exp2f(q);
    return x > 0.f ? x - r : r;
}

template <int BM, int BN, int kBK, bool B_KN, int WAVES_N = 2>
__global__ void __launch_bounds__(256) gemm_f32_kernel(GemmArgs g) {
    constexpr int LDA = BM + 4, LDB = BN + 4;  // k-major LDS rows; +4 keeps float4 alignment and staggers banks
    constexpr int WAVES_M = 4 / WAVES_N;
    constexpr int WM = BM / WAVES_M, WN = BN / WAVES_N, TM = WM / 32, TN = WN / 32;
    constexpr int A_F4 = BM * kBK / 4 / 256;  // float4 loads per thread per tile
    constexpr int B_F4 = (BN * kBK / 4 + 255) / 256;
    constexpr bool B_EXACT = BN * kBK / 4 % 256 == 0;   // 96-column tiles: 1.5 float4 per thread, the tail is guarded
    static_assert(A_F4 >= 1 && B_F4 >= 1 && WM % 32 == 0 && WN % 32 == 0, "tile / wave layout");
    __shared__ __attribute__((aligned(16))) float As[2][kBK][LDA];
    __shared__ __attribute__((aligned(16))) float Bs[2][kBK][LDB];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wr = wave / WAVES_N, wc = wave % WAVES_N;
    // XCD-aware tile order: hardware deals consecutive workgroup ids round-robin over the 8 XCDs; remap so that
    // each XCD walks a CONTIGUOUS run of tiles (n fastest) -- the column tiles that share an A row-tile then hit
    // that XCD's L2 instead of eight different ones.
    uint32_t bx, by, bz;
    {
        const uint32_t gx = gridDim.x, gy = gridDim.y, nb = gx * gy * gridDim.z;
        const uint32_t b = blockIdx.x + gx * (blockIdx.y + gy * blockIdx.z);
        const uint32_t x = b & 7, q8 = nb >> 3, r8 = nb & 7;
        const uint32_t L = x * q8 + (x < r8 ? x : r8) + (b >> 3);
        bx = L % gx;
        by = (L / gx) % gy;
        bz = L / (gx * gy);
    }
    const int m0 = by * BM, n0 = bx * BN;
    const int z1 = bz / g.nz2, z2 = bz % g.nz2;
    const float* A = g.A + z1 * g.sa1 + z2 * g.sa2;
    const float* B = g.B + z1 * g.sb1 + z2 * g.sb2;
    float* C = g.C + z1 * g.sc1 + z2 * g.sc2;

    float4 ra[A_F4], rb[B_F4];
    auto load_tiles = [&](int k0) {
#pragma unroll
        for (int p = 0; p < A_F4; ++p) {
            const int idx = tid + 256 * p, row = idx / (kBK / 4), k4 = idx % (kBK / 4);
            const int m = m0 + row, k = k0 + 4 * k4;
            ra[p] = (m < g.M && k < g.K) ? *reinterpret_cast<const float4*>(A + (size_t)m * g.lda + k)
                                         : make_float4(0.f, 0.f, 0.f, 0.f);
        }
#pragma unroll
        for (int p = 0; p < B_F4; ++p) {
            const int idx = tid + 256 * p;
            if constexpr (B_KN) {
                constexpr int N4 = BN / 4;
                const int kr = idx / N4, n4 = idx % N4;
                const int k = k0 + kr, n = n0 + 4 * n4;
                rb[p] = (k < g.K && n < g.N) ? *reinterpret_cast<const float4*>(B + (size_t)k * g.ldb + n)
                                             : make_float4(0.f, 0.f, 0.f, 0.f);
            } else {
                const int row = idx / (kBK / 4), k4 = idx % (kBK / 4);
                const int n = n0 + row, k = k0 + 4 * k4;
                rb[p] = ((B_EXACT || row < BN) && n < g.N && k < g.K) ? *reinterpret_cast<const float4*>(B + (size_t)n * g.ldb + k)
                                                                      : make_float4(0.f, 0.f, 0.f, 0.f);
            }
        }
    };
    auto store_tiles = [&](int buf) {
#pragma unroll
        for (int p = 0; p < A_F4; ++p) {
            const int idx = tid + 256 * p, row = idx / (kBK / 4), k4 = idx % (kBK / 4);
            As[buf][4 * k4 + 0][row] = ra[p].x;
            As[buf][4 * k4 + 1][row] = ra[p].y;
            As[buf][4 * k4 + 2][row] = ra[p].z;
            As[buf][4 * k4 + 3][row] = ra[p].w;
        }
#pragma unroll
        for (int p = 0; p < B_F4; ++p) {
            const int idx = tid + 256 * p;
            if constexpr (B_KN) {
                constexpr int N4 = BN / 4;
                const int kr = idx / N4, n4 = idx % N4;
                *reinterpret_cast<float4*>(&Bs[buf][kr][4 * n4]) = rb[p];
            } else {
                const int row = idx / (kBK / 4), k4 = idx % (kBK / 4);
                if (B_EXACT || row < BN) {
                    Bs[buf][4 * k4 + 0][row] = rb[p].x;
                    Bs[buf][4 * k4 + 1][row] = rb[p].y;
                    Bs[buf][4 * k4 + 2][row] = rb[p].z;
                    Bs[buf][4 * k4 + 3][row] = rb[p].w;
                }
            }
        }
    };

    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    const int nk = (g.K + kBK - 1) / kBK;
    load_tiles(0);
    store_tiles(0);
    __syncthreads();
    const int lr = lane & 31, lk = lane >> 5;
    for (int t = 0; t < nk; ++t) {
        const int buf = t & 1;
        if (t + 1 < nk) load_tiles((t + 1) * kBK);  // in flight under the MFMAs below
#pragma unroll
        // k-step kk multiplies k rows kk (lanes 0-31) and kk + 8 (lanes 32-63): any pairing of the 16 rows sums
        // to the same product, and this one puts the two half-waves on opposite halves of the 64 LDS banks
        // (8 rows x 132 floats = 32 mod 64), so the operand reads are conflict free.
        for (int kk = 0; kk < kBK / 2; ++kk) {
            float a[TM], b[TN];
#pragma unroll
            for (int i = 0; i < TM; ++i) a[i] = As[buf][kk + (kBK / 2) * lk][wr * WM + 32 * i + lr];
#pragma unroll
            for (int j = 0; j < TN; ++j) b[j] = Bs[buf][kk + (kBK / 2) * lk][wc * WN + 32 * j + lr];
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i], b[j], acc[i][j], 0, 0, 0);
        }
        if (t + 1 < nk) store_tiles(buf ^ 1);
        __syncthreads();
    }

    // epilogue: C/D layout of 32x32 MFMA: col = lane & 31, row = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5)
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            const int n = n0 + wc * WN + 32 * j + lr;
            if (n >= g.N) continue;
            const float bv = g.bias ? g.bias[n] : 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int m = m0 + wr * WM + 32 * i + (r & 3) + 8 * (r >> 2) + 4 * lk;
                if (m >= g.M) continue;
                float v = acc[i][j][r] * g.alpha + bv;
                if (g.gelu) v = gelu_erf(v);
                if (g.res) v += g.res[(size_t)m * g.ldr + n];
                C[(size_t)m * g.ldc + n] = v;
            }
        }
}

// ---------------------------------------------------------------------------------------------------------------------
// The same GEMM on the bf16 matrix pipe at fp32 accuracy ("bf16x3"): every fp32 operand is split into three bf16 planes,
// x = x1 + x2 + x3 (x1 = bf16(x), x2 = bf16(x - x1), x3 = bf16(x - x1 - x2): 24 mantissa bits, the two subtractions are
// exact), and a product a.b is accumulated as the six terms of order >= 2^-16: a1b1 + a1b2 + a2b1 + a1b3 + a2b2 + a3b1
// (the three dropped terms are <= 2^-24 |a||b|, fp32's own rounding).  v_mfma_f32_32x32x16_bf16 runs at 16x the rate of
// the fp32-input MFMA, so six of them cost 3/8 of the fp32 form's matrix-pipe time; accumulation is fp32 in both.
// Operands are split ONCE, when a tile is staged (registers -> three bf16 planes in LDS, each plane as two k halves of
// [row][8 bf16]: the 16-byte fragment reads are conflict free); A [M, K] and B [N, K] both k-contiguous (nn.Linear).
// ---------------------------------------------------------------------------------------------------------------------
typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));

template <int BM, int BN, int WAVES_N = 2>
__global__ void __launch_bounds__(256, 2) gemm_bf16x3_kernel(GemmArgs g) {
    constexpr int kBK = 16;
    constexpr int WAVES_M = 4 / WAVES_N;
    constexpr int WM = BM / WAVES_M, WN = BN / WAVES_N, TM = WM / 32, TN = WN / 32;
    constexpr int A_F4 = BM * kBK / 4 / 256;   // float4 loads per thread per tile
    constexpr int B_F4 = (BN * kBK / 4 + 255) / 256;
    constexpr bool B_EXACT = BN * kBK / 4 % 256 == 0;
    static_assert(A_F4 >= 1 && WM % 32 == 0 && WN % 32 == 0, "tile / wave layout");
    // [buffer][plane][k half][row][8 bf16]: a fragment read (lane = row, k half) is conflict free (ds_read_b128's lane groups
    // each cover 16 distinct rows = 256 bytes).  The staging stores (ds_write_b64: groups of 16 lanes = 4 rows x both k halves,
    // 32 store banks of 4 bytes) need the two k halves 64 bytes apart modulo 128: 64 bytes of padding behind each half (rows
    // x 16 B is a multiple of 128; unpadded every store was a 2-way conflict -- a third of the kernel's LDS cycles,
    // SQ_LDS_BANK_CONFLICT).  49.5 KB per workgroup: three still fit a CU.
    __shared__ __attribute__((aligned(16))) uint32_t As[2][3][2][BM * 4 + 16];
    __shared__ __attribute__((aligned(16))) uint32_t Bs[2][3][2][BN * 4 + 16];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wr = wave / WAVES_N, wc = wave % WAVES_N;
    uint32_t bx, by, bz;       // XCD-aware tile order, as gemm_f32_kernel
    {
        const uint32_t gx = gridDim.x, gy = gridDim.y, nb = gx * gy * gridDim.z;
        const uint32_t b = blockIdx.x + gx * (blockIdx.y + gy * blockIdx.z);
        const uint32_t x = b & 7, q8 = nb >> 3, r8 = nb & 7;
        const uint32_t L = x * q8 + (x < r8 ? x : r8) + (b >> 3);
        bx = L % gx;
        by = (L / gx) % gy;
        bz = L / (gx * gy);
    }
    const int m0 = by * BM, n0 = bx * BN;
    const int z1 = bz / g.nz2, z2 = bz % g.nz2;
    const float* A = g.A + z1 * g.sa1 + z2 * g.sa2;
    const float* B = g.B + z1 * g.sb1 + z2 * g.sb2;
    float* C = g.C + z1 * g.sc1 + z2 * g.sc2;

    // Pipeline (tile t is multiplied in iteration t): global loads run TWO tiles ahead (their latency is longer than one tile's
    // MFMAs), the split + LDS stores of tile t + 1 are threaded between the MFMAs of tile t (the matrix pipe takes 32
    // cycles per instruction on a SIMD: ~5 VALU issue slots per MFMA are free), one barrier per tile.
    struct Stage {
        float4 a[A_F4], b[B_F4];
    };
    // (rows past M / N are clamped, not predicated: they only feed output rows / columns that are never stored, and a
    // branch-free body lets the MFMAs and the staging arithmetic of a tile be scheduled as one block; K % 16 == 0)
    auto load_tiles = [&](Stage& r, int k0) {
#pragma unroll
        for (int p = 0; p < A_F4; ++p) {
            const int idx = tid + 256 * p, row = idx / (kBK / 4), k4 = idx % (kBK / 4);
            r.a[p] = *reinterpret_cast<const float4*>(A + (size_t)min(m0 + row, g.M - 1) * g.lda + k0 + 4 * k4);
        }
#pragma unroll
        for (int p = 0; p < B_F4; ++p) {
            const int idx = tid + 256 * p, row = idx / (kBK / 4), k4 = idx % (kBK / 4);
            r.b[p] = *reinterpret_cast<const float4*>(B + (size_t)min(n0 + row, g.N - 1) * g.ldb + k0 + 4 * k4);
        }
    };
    auto store_tiles = [&](const Stage& r, int buf) {
#pragma unroll
        for (int p = 0; p < A_F4; ++p) {
            const int idx = tid + 256 * p, row = idx / (kBK / 4), k4 = idx % (kBK / 4);
            uint32_t a1, a2, a3, b1, b2, b3;
            split3_bf16(r.a[p].x, r.a[p].y, a1, a2, a3);
            split3_bf16(r.a[p].z, r.a[p].w, b1, b2, b3);
            *reinterpret_cast<uint2*>(&As[buf][0][k4 >> 1][4 * row + 2 * (k4 & 1)]) = make_uint2(a1, b1);
            *reinterpret_cast<uint2*>(&As[buf][1][k4 >> 1][4 * row + 2 * (k4 & 1)]) = make_uint2(a2, b2);
            *reinterpret_cast<uint2*>(&As[buf][2][k4 >> 1][4 * row + 2 * (k4 & 1)]) = make_uint2(a3, b3);
        }
#pragma unroll
        for (int p = 0; p < B_F4; ++p) {
            const int idx = tid + 256 * p, row = idx / (kBK / 4), k4 = idx % (kBK / 4);
            if (B_EXACT || row < BN) {
                uint32_t a1, a2, a3, b1, b2, b3;
                split3_bf16(r.b[p].x, r.b[p].y, a1, a2, a3);
                split3_bf16(r.b[p].z, r.b[p].w, b1, b2, b3);
                *reinterpret_cast<uint2*>(&Bs[buf][0][k4 >> 1][4 * row + 2 * (k4 & 1)]) = make_uint2(a1, b1);
                *reinterpret_cast<uint2*>(&Bs[buf][1][k4 >> 1][4 * row + 2 * (k4 & 1)]) = make_uint2(a2, b2);
                *reinterpret_cast<uint2*>(&Bs[buf][2][k4 >> 1][4 * row + 2 * (k4 & 1)]) = make_uint2(a3, b3);
            }
        }
    };

    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    const int nk = (g.K + kBK - 1) / kBK;
    const int lr = lane & 31, lk = lane >> 5;
    Stage st0, st1;
    load_tiles(st0, 0);
    store_tiles(st0, 0);
    load_tiles(st0, min(1, nk - 1) * kBK);       // tile 1 -> st0, tile 2 -> st1, tile 3 -> st0, ...
    __syncthreads();
    auto tile_step = [&](int t, Stage& cur, Stage& nxt) {
        // cur holds tile t + 1 (loaded one iteration ago); tile t + 2 goes into nxt
        const int buf = t & 1;
        load_tiles(nxt, min(t + 2, nk - 1) * kBK);        // (past the end: the last tile again, unused)
        // fragments: lane = (row lr, k half lk): eight consecutive k of one row = one 16-byte read per plane; A and B use
        // the same (lane half, element) -> k map, which is all the instruction's sum over k needs
        bf16x8_t af[TM][3], bfr[TN][3];
#pragma unroll
        for (int pl = 0; pl < 3; ++pl) {
#pragma unroll
            for (int i = 0; i < TM; ++i)
                af[i][pl] = __builtin_bit_cast(bf16x8_t, *reinterpret_cast<const uint4*>(&As[buf][pl][lk][4 * (wr * WM + 32 * i + lr)]));
#pragma unroll
            for (int j = 0; j < TN; ++j)
                bfr[j][pl] = __builtin_bit_cast(bf16x8_t, *reinterpret_cast<const uint4*>(&Bs[buf][pl][lk][4 * (wc * WN + 32 * j + lr)]));
        }
        store_tiles(cur, buf ^ 1);                        // (after the last tile: into the idle buffer, unread)
        // the six products, smallest terms first; the TM x TN accumulators take turns inside each term
        constexpr int PA[6] = {2, 0, 1, 1, 0, 0}, PB[6] = {0, 2, 1, 0, 1, 0};
#pragma unroll
        for (int term = 0; term < 6; ++term)
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[i][PA[term]], bfr[j][PB[term]], acc[i][j], 0, 0, 0);
        // issue order: one MFMA, then the VALU / LDS-store work that fits its shadow
        __builtin_amdgcn_sched_group_barrier(0x020, A_F4 + B_F4, 0);      // the global loads first: they have two tiles to land
#pragma unroll
        for (int m = 0; m < 6 * TM * TN; ++m) {
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
            __builtin_amdgcn_sched_group_barrier(0x002, 5, 0);
            __builtin_amdgcn_sched_group_barrier(0x200, 1, 0);
        }
        __syncthreads();
    };
    for (int t = 0; t < nk; t += 2) {
        tile_step(t, st0, st1);
        if (t + 1 < nk) tile_step(t + 1, st1, st0);
    }

    // epilogue: C/D layout of 32x32 MFMA: col = lane & 31, row = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5)
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            const int n = n0 + wc * WN + 32 * j + lr;
            if (n >= g.N) continue;
            const float bv = g.bias ? g.bias[n] : 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int m = m0 + wr * WM + 32 * i + (r & 3) + 8 * (r >> 2) + 4 * lk;
                if (m >= g.M) continue;
                float v = acc[i][j][r] * g.alpha + bv;
                if (g.gelu) v = gelu_erf(v);
                if (g.res) v += g.res[(size_t)m * g.ldr + n];
                C[(size_t)m * g.ldc + n] = v;
            }
        }
}


// ---------------------------------------------------------------------------------------------------------------------
// Pre-split operands ("P layout") and the GEMM that streams them.  Round 2's bf16x3 kernel split BOTH fp32 operands into
// three bf16 planes on the fly, in every workgroup, for every tile (28 M VALU wave-instructions per 8192 x 2304 x 768
// launch) and paid SIX matrix instructions per term; the matrix pipe was busy 0.37 - 0.41 of the launch and throttled the
// clock.  Here the planes are formed ONCE -- the weights when the model is loaded (aspire_bert_prepare_planes), an activation
// by the epilogue of the kernel that produces it (LayerNorm, attention, the GELU GEMM) -- the GEMM's main loop is LDS-DMA +
// fragment reads + MFMAs, and the split is TWO fp16 planes:
//     x = h + l,  h = fp16(x) (round to nearest),  l = fp16(x - h):   |x - h - l| <= 2^-24 |x|  (11 + 11 bits and l's sign)
//     x . y = h.h' + h.l' + l.h'  (+ l.l' <= 2^-22 of the term: dropped)
// -- THREE v_mfma_f32_32x32x16_f16 per term, products exact, sums in fp32.  That is fp32's own precision as long as l does not
// lose bits to fp16's narrow exponent: the matrix pipe keeps fp16 subnormals (tools/experiments/mfma_f16_denorm.hip), so an l
// below 2^-14 still carries an absolute 2^-25 -- elements of magnitude >= 2^-3 are split at full relative precision and the
// rest at an absolute error below that of an fp32 sum of O(1) terms.  Activations (LayerNorm outputs, attention context, GELU
// outputs: O(1), far below fp16's 65504) go in as they are; the weights (~0.02 - 0.05) are scaled by kPWeightScale = 2^6
// before the split and the epilogue takes the factor off again (exact).  Measured against a float64 product at K = 768: rms
// error 0.2 x that of a plain fp32 GEMM's before accumulation (numpy model), tests/test_gpu_encoder.py on the device.
//
// P layout of a matrix X [R, K] (K % 32 == 0), 4 bytes per element: for every 16-wide k block kb and row r four 16-byte
// pieces (plane pl, k half kh) = the 8 fp16 of plane pl at k = 16 kb + 8 kh .. + 7, stored at
//     piece index (kb * R + r) * 4 + ((2 pl + kh) ^ ((r >> 2) & 3))
// so that (a) the 128 rows of a tile at one k block are ONE contiguous 8 KB run: eight global_load_lds_dwordx4 move it into
// LDS exactly as it lies in HBM (the LDS image of an LDS-DMA is lane-linear), and (b) a fragment read -- lane = (row, k half)
// reads 16 bytes -- is conflict free: 64-byte rows put rows r and r + 4 on the same banks, the XOR with the row's bits 2..3
// spreads the sixteen rows of a ds_read_b128 lane group over the sixteen 16-byte columns of the 256-byte bank line.
// ---------------------------------------------------------------------------------------------------------------------
constexpr int kPRowBytes = 64;                       // one row of one k block: 2 planes x 2 halves x 16 bytes
constexpr int kPTile = 128 * kPRowBytes;             // 128 rows of one k block (8 KB)
constexpr int kPPadRows = 256;                       // rows of slack behind a P matrix: the last row tile (128 or 256 rows) may read past R
constexpr int kPRingDefault = 13;                    // 10 KS + NS: stages of one k block, three-stage ring = 48 KB, three workgroups per CU
constexpr float kPWeightScale = 64.f;                // weights are split as 64 w (module comment)

typedef _Float16 f16x8_t __attribute__((ext_vector_type(8)));

// Timing probes of gemm_p_kernel (ASPIRE_HIP_GEMM_PROBE; wrong results by design) exist only in builds with -DASPIRE_GEMM_PROBES
// (probes alone) or -DASPIRE_PHASE_CLOCK (probes + time stamps, tools/build_clock.sh; the stamps themselves cost ~30 %):
// 1 no MFMAs, 2 no LDS-DMA, 3 every workgroup computes tile (0, 0) (operands always cache-hot), 4 no epilogue, 5 / 6 = 1 / 2
// without epilogue, 10 no B-tile DMA and no epilogue, 11 LDS-DMA + fragment reads only, 20 stamps inside step 8.
#if defined(ASPIRE_PHASE_CLOCK) || defined(ASPIRE_GEMM_PROBES)
#define G_PROBE(g) ((g).probe)
#else
#define G_PROBE(g) 0
#endif

#ifdef ASPIRE_PHASE_CLOCK
// debug build only (tools/gemmphases.py): per-workgroup time stamps (100 MHz wall clock) of gemm_p_kernel into the buffer set by
// aspire_debug_gemm_buffer: [workgroup][16] = start, first tile landed, main loop done, stores issued, HW_ID, XCC_ID, -, -,
// then inside step 8: after its barrier, after its LDS-DMA issue, after its MFMAs' issue, step 9: after its vmcnt wait, after its barrier
static __device__ long long* g_gdbg = nullptr;
#define G_STAMP(k, v)                                                                                                \
    do {                                                                                                             \
        if (g_gdbg && threadIdx.x == 0) g_gdbg[(size_t)(blockIdx.x + gridDim.x * blockIdx.y) * 16 + (k)] = (long long)(v); \
    } while (0)
#else
#define G_STAMP(k, v) \
    do {              \
    } while (0)
#endif

__host__ __device__ inline size_t p_bytes(int64_t R, int64_t K) { return (size_t)(R + kPPadRows) * K * 4; }

// eight values -> the two planes' 16-byte pieces
__device__ __forceinline__ void split8_f16(const float (&v)[8], f16x8_t& h, f16x8_t& l) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const _Float16 hj = (_Float16)v[j];
        h[j] = hj;
        l[j] = (_Float16)(v[j] - (float)hj);
    }
}

// (x, y) -> packed fp16 pairs of the two planes
__device__ __forceinline__ void split2_f16(float x, float y, uint32_t& h, uint32_t& l) {
    const _Float16 hx = (_Float16)x, hy = (_Float16)y;
    const _Float16 lx = (_Float16)(x - (float)hx), ly = (_Float16)(y - (float)hy);
    h = (uint32_t)__builtin_bit_cast(uint16_t, hx) | ((uint32_t)__builtin_bit_cast(uint16_t, hy) << 16);
    l = (uint32_t)__builtin_bit_cast(uint16_t, lx) | ((uint32_t)__builtin_bit_cast(uint16_t, ly) << 16);
}

// four consecutive k (k % 4 == 0) of row r -> the two planes' 8-byte halves
__device__ __forceinline__ void p_store4(void* P, int64_t R, int64_t r, int k, float x, float y, float z, float w) {
    uint32_t h0, l0, h1, l1;
    split2_f16(x, y, h0, l0);
    split2_f16(z, w, h1, l1);
    const int kb = k >> 4, kh = (k >> 3) & 1, half = (k >> 2) & 1, sw = (int)((r >> 2) & 3);
    char* row = (char*)P + ((size_t)kb * R + r) * kPRowBytes + half * 8;
    *reinterpret_cast<uint2*>(row + 16 * (kh ^ sw)) = make_uint2(h0, h1);
    *reinterpret_cast<uint2*>(row + 16 * ((2 + kh) ^ sw)) = make_uint2(l0, l1);
}

// (the LayerNorm epilogue's form of the two: byte offsets in 32 bits from the uniform base -- a P matrix is far below 4 GB -- so that the
// sixteen slots a lane reads and later rewrites cost sixteen registers of addresses, not sixty-four)
__device__ __forceinline__ uint32_t p_slot(uint32_t R, uint32_t r, uint32_t k) {
    return (((k >> 4) * R + r) << 6) + ((k >> 2) & 1) * 8 + 16 * (((k >> 3) & 1) ^ ((r >> 2) & 3));      // the h plane's 8 bytes; l: ^ 32
}
__device__ __forceinline__ float4 p_load4_at(const void* P, uint32_t slot) {
    const uint2 h = *reinterpret_cast<const uint2*>((const char*)P + slot), l = *reinterpret_cast<const uint2*>((const char*)P + (slot ^ 32u));
    typedef _Float16 h2 __attribute__((ext_vector_type(2)));
    const h2 h0 = __builtin_bit_cast(h2, h.x), h1 = __builtin_bit_cast(h2, h.y), l0 = __builtin_bit_cast(h2, l.x), l1 = __builtin_bit_cast(h2, l.y);
    return make_float4((float)h0.x + (float)l0.x, (float)h0.y + (float)l0.y, (float)h1.x + (float)l1.x, (float)h1.y + (float)l1.y);
}
__device__ __forceinline__ void p_store4_at(void* P, uint32_t slot, float x, float y, float z, float w) {
    uint32_t h0, l0, h1, l1;
    split2_f16(x, y, h0, l0);
    split2_f16(z, w, h1, l1);
    *reinterpret_cast<uint2*>((char*)P + slot) = make_uint2(h0, h1);
    *reinterpret_cast<uint2*>((char*)P + (slot ^ 32u)) = make_uint2(l0, l1);
}

// EIGHT consecutive k (k % 8 == 0) of row r: one whole 16-byte piece per plane
__device__ __forceinline__ uint32_t p_slot8(uint32_t R, uint32_t r, uint32_t k) {
    return (((k >> 4) * R + r) << 6) + 16 * (((k >> 3) & 1) ^ ((r >> 2) & 3));      // the h plane's piece; l: ^ 32
}
__device__ __forceinline__ void p_load8_at(const void* P, uint32_t slot, float (&x)[8]) {
    const f16x8_t h = *reinterpret_cast<const f16x8_t*>((const char*)P + slot), l = *reinterpret_cast<const f16x8_t*>((const char*)P + (slot ^ 32u));
#pragma unroll
    for (int c = 0; c < 8; ++c) x[c] = (float)h[c] + (float)l[c];
}
__device__ __forceinline__ void p_store8_at(void* P, uint32_t slot, const float (&x)[8]) {
    f16x8_t h, l;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        const _Float16 t = (_Float16)x[c];
        h[c] = t;
        l[c] = (_Float16)(x[c] - (float)t);
    }
    *reinterpret_cast<f16x8_t*>((char*)P + slot) = h;
    *reinterpret_cast<f16x8_t*>((char*)P + (slot ^ 32u)) = l;
}

// ... and back: h + l of four consecutive k of row r (what p_store4 wrote, to 2^-24 relative / 2^-25 absolute: fp32's own rounding)
__device__ __forceinline__ float4 p_load4(const void* P, int64_t R, int64_t r, int k) {
    const int kb = k >> 4, kh = (k >> 3) & 1, half = (k >> 2) & 1, sw = (int)((r >> 2) & 3);
    const char* row = (const char*)P + ((size_t)kb * R + r) * kPRowBytes + half * 8;
    const uint2 h = *reinterpret_cast<const uint2*>(row + 16 * (kh ^ sw)), l = *reinterpret_cast<const uint2*>(row + 16 * ((2 + kh) ^ sw));
    typedef _Float16 h2 __attribute__((ext_vector_type(2)));
    const h2 h0 = __builtin_bit_cast(h2, h.x), h1 = __builtin_bit_cast(h2, h.y), l0 = __builtin_bit_cast(h2, l.x), l1 = __builtin_bit_cast(h2, l.y);
    return make_float4((float)h0.x + (float)l0.x, (float)h0.y + (float)l0.y, (float)h1.x + (float)l1.x, (float)h1.y + (float)l1.y);
}

// *too_big (optional) is raised when an element leaves fp16's range (|scale x| > 65504, or not finite)
__global__ void __launch_bounds__(256) split_planes_kernel(const float* __restrict__ X, int64_t R, int K, int ld, void* __restrict__ P,
                                                           float scale, int* __restrict__ too_big) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int k4 = K / 4;
    if (idx >= R * k4) return;
    const int64_t r = idx / k4;
    const int k = (int)(idx % k4) * 4;
    const float4 v = *reinterpret_cast<const float4*>(X + r * ld + k);
    p_store4(P, R, r, k, scale * v.x, scale * v.y, scale * v.z, scale * v.w);
    if (too_big && !(fmaxf(fmaxf(fabsf(v.x), fabsf(v.y)), fmaxf(fabsf(v.z), fabsf(v.w))) * scale <= 65504.f)) *too_big = 1;
}

// Sticky per-device status word of the encoder's kernels (include/aspire_hip.h: aspire_bert_status reads and clears it).
__device__ int g_bert_status;
// how long a LayerNorm-epilogue tile waits for its row block's partners: 20 ms of the constant 100 MHz clock (s_memrealtime) -- two orders
// of magnitude above the longest kernel any stream of this library keeps the chip busy with, so that only a broken progress assumption
// (not a busy GPU) runs into it
constexpr uint64_t kLnWaitTicks = 2000000;

struct PGemmArgs {
    const void* Ap;      // P layout [M, K]
    const void* Bp;      // P layout [N, K] (nn.Linear weight, scaled by kPWeightScale)
    float* C;            // fp32 [M, ldc] out (F32 epilogue)
    void* Cp;            // P layout [M, N] out (GELU_P epilogue: the next GEMM's A operand, its k dimension = N)
    const float* bias;   // [N] or null
    const float* res;    // [M, ldr] residual or null
    int M, N, K, ldc, ldr;
    int n_off;           // first column of this launch (a GEMM may run as a launch of 128-wide and one of 64-wide column tiles)
    int probe;           // timing probes (ASPIRE_HIP_GEMM_PROBE): 1 no MFMAs, 2 no LDS-DMA
    int tiles_x, tiles_y;   // PERSIST / LN: the tile grid (PERSIST: a workgroup walks several tiles; the launch grid is the resident workgroups)
    // LN epilogue (N = 768 = the whole row): y = LayerNorm(acc + bias + residual) * gamma + beta -> C (fp32, optional) and Cp (P layout,
    // optional); the residual is READ from a P layout [M, 768] (resp; h + l = the fp32 value to fp32's own rounding) and may BE Cp:
    // every 8-byte slot is read and later written by the one lane that owns it
    const void* resp;
    const float *gamma, *beta;
    float eps;
    float2* ln_stats;    // [M][768 / BN] (mean, sum of squared deviations) of a row's BN columns, one entry per column tile
    int* ln_count;       // [row blocks] zeroed before the launch: column tiles of the row block that have published their entry
    // QKV epilogue (EPI 1, launch_gemm_p_qkv): the attention kernel's operands, already split -- Xp = the planes
    // [plane h | l][Q | K | V][head][M][64] fp16 (flash_attn_p_kernel)
    void* Xp;
};

// One 16-byte-per-lane LDS-DMA: 64 lanes x 16 B from global bytes [base + IMM + voff(lane)] to LDS bytes [lds_dst + IMM, .. + 1024).
// The address is a uniform 64-bit base in SGPRs plus a per-lane 32-bit offset that never changes (16 lane): stepping along k
// is scalar arithmetic only -- with per-lane 64-bit addresses every issue paid a v_lshl_add_u64 that queues behind the other
// workgroup's MFMAs on the same SIMD (measured with the phase stamps: 8 issues took 0.6 us of a 1.6 us step).  hipcc does not
// count this load: the caller waits with s_waitcnt vmcnt(N) itself.
// M0 is compiler-reserved: saved and restored inside the statement.  The pieces of one k block go out in ONE statement (two
// 1 KB pieces of A, TWO_B ? two : one of B): everything a wave issues in front of its fragment reads queues behind the MFMAs
// its neighbour on the SIMD is streaming (a handful of issue slots per 32-cycle MFMA), so the count matters: 13 (11)
// instructions per k block instead of 20 (15).
template <bool TWO_B>
__device__ __forceinline__ void glds_kblock(uint64_t a_base, uint64_t b_base, uint32_t voff, uint32_t a_dst, uint32_t b_dst) {
    uint32_t keep;
    if constexpr (TWO_B)
        asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %4\n\ts_nop 0\n\t"
                     "global_load_lds_dwordx4 %1, %2 offset:0\n\tglobal_load_lds_dwordx4 %1, %2 offset:1024\n\t"
                     "s_mov_b32 m0, %5\n\ts_nop 0\n\t"
                     "global_load_lds_dwordx4 %1, %3 offset:0\n\tglobal_load_lds_dwordx4 %1, %3 offset:1024\n\t"
                     "s_mov_b32 m0, %0"
                     : "=&s"(keep)
                     : "v"(voff), "s"(a_base), "s"(b_base), "s"(a_dst), "s"(b_dst)
                     : "memory");
    else
        asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %4\n\ts_nop 0\n\t"
                     "global_load_lds_dwordx4 %1, %2 offset:0\n\tglobal_load_lds_dwordx4 %1, %2 offset:1024\n\t"
                     "s_mov_b32 m0, %5\n\ts_nop 0\n\t"
                     "global_load_lds_dwordx4 %1, %3 offset:0\n\t"
                     "s_mov_b32 m0, %0"
                     : "=&s"(keep)
                     : "v"(voff), "s"(a_base), "s"(b_base), "s"(a_dst), "s"(b_dst)
                     : "memory");
}

// C = A . B^T on 128 x 128 tiles, four waves of 64 x 64, three fp16 products per term.  A stage = KS 16-wide k blocks (KS MFMA k
// steps); NS-stage LDS ring filled by LDS-DMA NS - 1 stages ahead; per stage and wave: 4 KS DMA pieces, 8 KS fragment reads,
// 12 KS MFMAs, one barrier.  Order of a step: wait for the own pieces of stage t (s_waitcnt vmcnt(kPerWave x the younger stages
// in flight)), barrier (everybody's pieces of stage t have landed AND everybody has read stage t - 1, whose slot is free now),
// issue stage t + NS - 1 into that slot, read fragments, multiply.
// SWAP: the MFMA's operands exchanged -- accumulator registers run along n, the lane is a row m -- for the epilogue that writes
// GELU(.) straight into the P layout of the next GEMM's A operand (a lane then holds 4 consecutive k of its row: one 8-byte
// store per plane); otherwise registers run along m, lanes along n: 128-byte coalesced fp32 stores, bias / residual fused.
// BN = 64: 128 x 64 tiles (wave tile 64 x 32) for the columns that would otherwise leave a last round of workgroups half empty.
// PERSIST (K / 16 a multiple of NS): the launch is the RESIDENT workgroups (three per CU) and a workgroup walks its XCD's share of
// the tiles; the k-block stream runs on across a tile boundary -- the first NS - 1 stages of the NEXT tile go out during the last
// steps of this one and land under its epilogue's stores, so a tile's prologue (address set-up, the first DMA round trips, the
// workgroup's own launch) is paid once per workgroup instead of once per tile.
// LN (SWAP form, N = 768): the 768 / BN workgroups of a row block exchange their rows' partial moments through global memory and each
// normalises its own 128 x BN block out of its accumulators -- no separate LayerNorm pass over [M, 768], no fp32 round trip of the
// pre-norm rows.  A workgroup WAITS for its row block's other column tiles: they are consecutive in the launch order of ONE XCD (below),
// the hardware starts workgroups in order, so whatever waits has all its partners started or next in line; the tiles that can be
// waiting at any time are the <= 8 row blocks at the launch frontier.
// BM = 256 (eight waves, 4 x 2 of 64 x 64; two workgroups per CU = four waves per SIMD): the A tile of a k block is 16 KB, every wave still
// moves two 1 KB pieces of it and ONE of B -- 24 KB of LDS-DMA per k block for 24 k-steps' worth of MFMAs per wave pair where two 128 x 128
// tiles move 32 KB: a quarter less traffic through the CU's vector-memory path and LDS per product.
template <int NS, int KS, int BN, bool SWAP, bool PERSIST = false, bool LN = false, int BM = 128, int EPI = 0>
__device__ __forceinline__ void gemm_p_body(const PGemmArgs& g) {
    static_assert(BM == 128 || (BM == 256 && !PERSIST && !LN), "tile rows");
    static_assert(EPI == 0 || (EPI == 1 && BM == 128 && BN == 128 && !PERSIST && !LN && SWAP), "QKV epilogue: 128 x 128 tiles, swapped orientation");
    constexpr int kATile = BM * kPRowBytes;                 // A rows of one k block
    static_assert(!PERSIST || KS == 1, "persistent form: one k block per stage");
    static_assert(!LN || (SWAP && !PERSIST && KS == 1), "LayerNorm epilogue: swapped operands, one tile per workgroup");
    constexpr int TN = BN / 64;                             // 32-column blocks per wave
    constexpr int kBTile = BN * kPRowBytes;                 // B rows of one k block
    constexpr int kStage = KS * (kATile + kBTile);          // [A k block 0 .. KS - 1][B k block 0 .. KS - 1]
    constexpr int kBPerWave = kBTile / (32 * BM);           // 1 KB pieces per wave and k block: 2 (128 x 128) or 1
    constexpr int kPerWave = KS * (2 + kBPerWave);          // LDS-DMA instructions per wave and stage
    extern __shared__ __attribute__((aligned(16))) unsigned char p_smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wave >> 1, wc = wave & 1, lr = lane & 31, lk = lane >> 5;
    // XCD-aware tile order, as gemm_f32_kernel: XCD x = workgroup id mod 8 owns a contiguous run of the tile sequence.  PERSIST: the
    // workgroups of an XCD share its run round-robin (tile_i = this workgroup's place among them, + tile_stride per tile)
    const uint32_t gx = PERSIST ? (uint32_t)g.tiles_x : gridDim.x, nb = gx * (PERSIST ? (uint32_t)g.tiles_y : gridDim.y);
    const uint32_t wg = blockIdx.x + gridDim.x * blockIdx.y;
    const uint32_t xcd = wg & 7, q8 = nb >> 3, r8 = nb & 7;
    const uint32_t tile_lo = xcd * q8 + (xcd < r8 ? xcd : r8), tile_n = PERSIST ? q8 + (xcd < r8 ? 1u : 0u) : 0u;
    const uint32_t tile_stride = PERSIST ? (gridDim.x - xcd + 7) >> 3 : 0u;
    uint32_t tile_i = wg >> 3;
    if (PERSIST && tile_i >= tile_n) return;
    uint32_t bx = (tile_lo + tile_i) % gx, by = (tile_lo + tile_i) / gx;
    if constexpr (LN) {
        // whole row blocks per XCD: XCD x takes row blocks [rb_lo, rb_lo + rb_n), its workgroups (wg = x, x + 8, ..) walk them column tile by column tile
        const uint32_t ty = (uint32_t)g.tiles_y, rq = ty >> 3, rr = ty & 7;
        const uint32_t rb_lo = xcd * rq + (xcd < rr ? xcd : rr), rb_n = rq + (xcd < rr ? 1u : 0u);
        if (tile_i >= rb_n * (uint32_t)g.tiles_x) return;
        by = rb_lo + tile_i / (uint32_t)g.tiles_x;
        bx = tile_i % (uint32_t)g.tiles_x;
    }
    int m0 = G_PROBE(g) == 3 ? 0 : (int)by * BM, n0 = G_PROBE(g) == 3 ? g.n_off : g.n_off + (int)bx * BN;      // probe 3: every workgroup computes tile (0, 0)
    G_STAMP(0, __builtin_amdgcn_s_memrealtime());
    G_STAMP(4, __builtin_amdgcn_s_getreg(31 << 11 | 4));
    G_STAMP(5, __builtin_amdgcn_s_getreg(31 << 11 | 20));
    const int nk = g.K / (16 * KS);
    const uint32_t lds0 = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) unsigned char*)p_smem;
    // per k block wave w moves pieces 2 w, 2 w + 1 (1 KB = 16 rows each) of the A rows and pieces 2 w, 2 w + 1 (BN = 64: piece w) of B's
    const uint64_t a_wave = (uint64_t)(uintptr_t)g.Ap + (2 * wave) * 1024, b_wave = (uint64_t)(uintptr_t)g.Bp + (kBPerWave * wave) * 1024;
    uint64_t a_src = a_wave + (uint64_t)m0 * kPRowBytes, b_src = b_wave + (uint64_t)n0 * kPRowBytes;
    uint64_t a_nxt = 0, b_nxt = 0;                            // PERSIST: the same of the workgroup's next tile
    const uint64_t a_step = (uint64_t)g.M * kPRowBytes, b_step = (uint64_t)g.N * kPRowBytes;
    const uint32_t lane16 = lane * 16;
    auto issue_from = [&](uint64_t a_from, uint64_t b_from, int slot, int t) {
        const uint32_t dst = lds0 + slot * kStage;
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            const uint64_t kb = (uint64_t)t * KS + s;
            // (an instruction's offset moves the LDS address along with the global one)
            glds_kblock<kBPerWave == 2>(a_from + kb * a_step, b_from + kb * b_step, lane16, dst + s * kATile + (2 * wave) * 1024,
                                        dst + KS * kATile + s * kBTile + (kBPerWave * wave) * 1024);
        }
    };
    auto issue = [&](int slot, int t) { issue_from(a_src, b_src, slot, t); };
    // fragment (plane pl) of this lane's row in a k block: piece (2 pl + lk) ^ ((row >> 2) & 3); the row's bits 2..3 are lr's (tiles
    // and wave tiles start on multiples of 32)
    const uint32_t frag0 = 16 * (lk ^ ((lr >> 2) & 3));
    const unsigned char* a_rd = p_smem + (wr * 64 + lr) * kPRowBytes;
    const unsigned char* b_rd = p_smem + KS * kATile + (wc * 32 * TN + lr) * kPRowBytes;

    f32x16 acc[2][TN];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
    // LN: the tile's bias values in LDS from the start (visible behind the first k step's barrier; read by the epilogue)
    __shared__ float4 ln_bias[LN ? BN / 4 : 1];
    if constexpr (LN) {
        if (tid < BN / 4) ln_bias[tid] = *reinterpret_cast<const float4*>(g.bias + n0 + 4 * tid);
    }

#pragma unroll
    for (int s = 0; s < NS - 1; ++s)
        if (s < nk) issue(s, s);
    bool first_tile = true, has_next = false;
    (void)first_tile;
    struct Frags {
        f16x8_t a[2][2][KS], b[TN][2][KS];       // [block][plane][k step]
    };
    auto read_frags = [&](Frags& f, int slot) {
#pragma unroll
        for (int s = 0; s < KS; ++s)           // the first MFMA k step's fragments first: its products start while the second's land
#pragma unroll
            for (int pl = 0; pl < 2; ++pl) {
                const uint32_t fo = frag0 ^ (32 * pl);
#pragma unroll
                for (int i = 0; i < 2; ++i)
                    f.a[i][pl][s] = __builtin_bit_cast(f16x8_t, *reinterpret_cast<const uint4*>(a_rd + slot * kStage + s * kATile + i * 32 * kPRowBytes + fo));
#pragma unroll
                for (int j = 0; j < TN; ++j)
                    f.b[j][pl][s] = __builtin_bit_cast(f16x8_t, *reinterpret_cast<const uint4*>(b_rd + slot * kStage + s * kBTile + j * 32 * kPRowBytes + fo));
            }
    };
    auto mma = [&](const Frags& f) {
        constexpr int PA[3] = {1, 0, 0}, PB[3] = {0, 1, 0};        // the small products first
#pragma unroll
        for (int s = 0; s < KS; ++s)
#pragma unroll
            for (int term = 0; term < 3; ++term)
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int j = 0; j < TN; ++j) {
                        if constexpr (SWAP)
                            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(f.b[j][PB[term]][s], f.a[i][PA[term]][s], acc[i][j], 0, 0, 0);
                        else
                            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(f.a[i][PA[term]][s], f.b[j][PB[term]][s], acc[i][j], 0, 0, 0);
                    }
    };
    static_assert(NS >= 2 && NS <= 4 && kPerWave * (NS - 2) < 64, "ring depth");
    auto step = [&](int t, int slot) {
        // the own pieces of stage t: everything but the younger stages' pieces (NS - 2 of them, fewer at the end of the loop --
        // PERSIST: of the workgroup's last tile).  PERSIST, a later tile's first NS - 1 stages: waited for in front of the previous
        // tile's epilogue (whose stores count in vmcnt too and may be acknowledged late: a vmcnt(N) here would wait for them).
        // lgkmcnt(0): this wave's fragment reads of the previous stage are done before anybody may refill that slot.
        const int younger = (PERSIST && has_next) || nk - 1 - t >= NS - 2 ? NS - 2 : nk - 1 - t;
        if (PERSIST && !first_tile && t < NS - 1) asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        else if (NS >= 4 && younger == 2) asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(2 * kPerWave) : "memory");
        else if (NS >= 3 && younger == 1) asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(kPerWave) : "memory");
        else asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
        if (G_PROBE(g) == 20 && t == 9) G_STAMP(11, __builtin_amdgcn_s_memrealtime());
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        if (t == 0) G_STAMP(1, __builtin_amdgcn_s_memrealtime());
        if (G_PROBE(g) == 20 && t == 8) G_STAMP(8, __builtin_amdgcn_s_memrealtime());
        if (G_PROBE(g) == 20 && t == 9) G_STAMP(12, __builtin_amdgcn_s_memrealtime());
        if (t + NS - 1 < nk) {
            if (G_PROBE(g) != 2 && G_PROBE(g) != 6) issue((slot + NS - 1) % NS, t + NS - 1);
        } else if (PERSIST && has_next) {
            issue_from(a_nxt, b_nxt, (slot + NS - 1) % NS, t + NS - 1 - nk);      // the next tile's first stages (nk % NS == 0: its stage s lives in slot s)
        }
        if (G_PROBE(g) == 20 && t == 8) G_STAMP(9, __builtin_amdgcn_s_memrealtime());
        Frags f;
        read_frags(f, slot);
        // all 8 KS fragment reads go out before the first MFMA (left alone the compiler reads four fragments at a time into the
        // same registers: six exposed LDS round trips per stage)
        __builtin_amdgcn_sched_barrier(0);
        if (G_PROBE(g) == 11) {         // LDS-DMA + fragment reads, no MFMAs
#pragma unroll
            for (int s = 0; s < KS; ++s)
#pragma unroll
                for (int pl = 0; pl < 2; ++pl) {
#pragma unroll
                    for (int i = 0; i < 2; ++i) asm volatile("" ::"v"(f.a[i][pl][s]));
#pragma unroll
                    for (int j = 0; j < TN; ++j) asm volatile("" ::"v"(f.b[j][pl][s]));
                }
        } else if (G_PROBE(g) != 1 && G_PROBE(g) != 5) mma(f);
        if (G_PROBE(g) == 20 && t == 8) G_STAMP(10, __builtin_amdgcn_s_memrealtime());
    };
    // the tile's bias values: fetched in front of the epilogue -- PERSIST: when the tile begins (no load may sit between one tile's
    // stores and the next tile's first steps: whoever waits for it waits for every store's acknowledgement, vmcnt counts both)
    float bias_n[TN];
    float4 bias_m[TN][4];
    auto load_bias = [&]() {       // (one uniform branch around ALL the loads: a per-value select would wait for each load where it is issued)
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            bias_n[j] = 0.f;
#pragma unroll
            for (int q4 = 0; q4 < 4; ++q4) bias_m[j][q4] = make_float4(0.f, 0.f, 0.f, 0.f);
        }
        if (!PERSIST && g.bias == nullptr) return;       // PERSIST: the launcher insists on a bias (a join behind the branch makes the compiler wait for the loads there)
        if constexpr (!SWAP) {
#pragma unroll
            for (int j = 0; j < TN; ++j) bias_n[j] = g.bias[n0 + wc * 32 * TN + 32 * j + lr];
        } else {
#pragma unroll
            for (int j = 0; j < TN; ++j)
#pragma unroll
                for (int q4 = 0; q4 < 4; ++q4) bias_m[j][q4] = *reinterpret_cast<const float4*>(g.bias + n0 + wc * 32 * TN + 32 * j + 8 * q4 + 4 * lk);
        }
    };
    if constexpr (PERSIST) load_bias();
  for (;;) {            // PERSIST: the workgroup's tiles; otherwise once
    if constexpr (PERSIST) {
        has_next = tile_i + tile_stride < tile_n;
        if (has_next) {
            const uint32_t L = tile_lo + tile_i + tile_stride;
            a_nxt = a_wave + (uint64_t)((L / gx) * 128) * kPRowBytes;
            b_nxt = b_wave + (uint64_t)(g.n_off + (int)(L % gx) * BN) * kPRowBytes;
        }
    }
    if constexpr (PERSIST) {
        static_assert(!PERSIST || NS == 3, "persistent form: the default ring");
#pragma unroll 1
        for (int t = 0; t < nk; t += 3) {
            step(t, 0);
            step(t + 1, 1);
            step(t + 2, 2);
        }
    } else {
        for (int t = 0; t < nk; t += NS) {
#pragma unroll
            for (int s = 0; s < NS; ++s)
                if (t + s < nk) step(t + s, s);
        }
    }
    // PERSIST: this wave's pieces of the next tile's first stages have landed before its stores go out (see step)
    if (PERSIST && has_next) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");

    G_STAMP(2, __builtin_amdgcn_s_memrealtime());
    constexpr float kUnscale = 1.0f / kPWeightScale;
    if constexpr (!PERSIST && !LN) load_bias();       // (LN: fetched block by block beside the residual)
    // every bias register is consumed HERE, in front of the first store: the compiler waits for the bias loads once, now, instead of
    // in front of the first use of each -- behind stores, where it can only wait with vmcnt(0) = for every store's acknowledgement
    if constexpr (LN) {
    } else if constexpr (!SWAP) {
#pragma unroll
        for (int j = 0; j < TN; ++j) asm volatile("" : "+v"(bias_n[j]));
    } else {
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int q4 = 0; q4 < 4; ++q4)
                asm volatile("" : "+v"(bias_m[j][q4].x), "+v"(bias_m[j][q4].y), "+v"(bias_m[j][q4].z), "+v"(bias_m[j][q4].w));
    }
    if (((G_PROBE(g) >= 4 && G_PROBE(g) <= 6) || (G_PROBE(g) >= 10 && G_PROBE(g) < 20)) && acc[0][0][0] != 12345.678f) return;      // probes 4+: no epilogue (4: all else, 5: no MFMAs, 6: no LDS-DMA)
    if constexpr (LN) {
        // lane = row m (col = lane & 31 of the swapped product), registers along n in groups of 4 columns, the lane pair (lk) interleaved:
        // n = 8 g + 4 lk + e.  One v_permlane32_swap per register pair first: lane half lk then holds columns 16 t + 8 lk + 0 .. 7 (t = 0, 1) of a
        // 32-column block in registers 8 t .. 8 t + 7 -- one whole 16-byte piece per plane and 16-column k block: the residual comes in and the
        // normalised row goes out in 16-byte accesses (8-byte ones before: 150 -> 147 us per launch at 16 384 rows).
        // A lane holds kCnt = 16 TN values of each of its two rows.  Moments are combined pairwise as (mean, M2 = sum of squared deviations) of
        // equal-sized groups: M2 = M2a + M2b + (n / 2) (mean_a - mean_b)^2 -- no E[x^2] - E[x]^2 cancellation anywhere.
        constexpr int kCnt = 16 * TN, kGX = kD / BN;
        // The residual's planes of BOTH 32-row blocks go out in one batch (16 x 16-byte loads per lane: 64 registers in flight; round 5 fetched one
        // 32-column block at a time -- four dependent round trips per tile at the end of a launch whose every tile is in this phase at once); the bias
        // comes from LDS (staged when the tile begins: no global load sits in this phase beside the residual's).  Issued FIRST: the register-pair
        // exchange below runs under the loads' flight.
        f16x8_t rh[2][TN][2], rl[2][TN][2];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int mc = min(m0 + wr * 64 + 32 * i + lr, g.M - 1);
#pragma unroll
            for (int j = 0; j < TN; ++j)
#pragma unroll
                for (int t = 0; t < 2; ++t) {
                    const uint32_t slot = p_slot8((uint32_t)g.M, (uint32_t)mc, (uint32_t)(n0 + wc * 32 * TN + 32 * j + 16 * t + 8 * lk));
                    rh[i][j][t] = *reinterpret_cast<const f16x8_t*>((const char*)g.resp + slot);
                    rl[i][j][t] = *reinterpret_cast<const f16x8_t*>((const char*)g.resp + (slot ^ 32u));
                }
        }
        __builtin_amdgcn_sched_barrier(0);       // (left alone the scheduler sinks the loads to their uses again, four at a time)
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j)
#pragma unroll
                for (int t = 0; t < 2; ++t) {
                    float lo[4], hi[4];
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        // (scalars first, both ways: a bit_cast applied to a vector ELEMENT reads element 0 with this clang)
                        const float fa = acc[i][j][8 * t + e], fb = acc[i][j][8 * t + 4 + e];
                        auto r = __builtin_amdgcn_permlane32_swap(__builtin_bit_cast(int, fa), __builtin_bit_cast(int, fb), false, false);
                        const int x0 = r[0], x1 = r[1];
                        lo[e] = __builtin_bit_cast(float, x0);
                        hi[e] = __builtin_bit_cast(float, x1);
                    }
#pragma unroll
                    for (int e = 0; e < 4; ++e) acc[i][j][8 * t + e] = lo[e], acc[i][j][8 * t + 4 + e] = hi[e];
                }
        float mu[2], m2[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            float s = 0.f;
#pragma unroll
            for (int j = 0; j < TN; ++j) {
#pragma unroll
                for (int t = 0; t < 2; ++t) {
                    const int c4 = (wc * 32 * TN + 32 * j + 16 * t + 8 * lk) >> 2;
                    const float4 b0 = ln_bias[c4], b1 = ln_bias[c4 + 1];
                    const float b8[8] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
#pragma unroll
                    for (int c = 0; c < 8; ++c) {
                        const float x = fmaf(acc[i][j][8 * t + c], kUnscale, b8[c]) + ((float)rh[i][j][t][c] + (float)rl[i][j][t][c]);
                        acc[i][j][8 * t + c] = x;
                        s += x;
                    }
                }
            }
            const float ml = s * (1.0f / kCnt);
            float q = 0.f;
#pragma unroll
            for (int j = 0; j < TN; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const float d = acc[i][j][r] - ml;
                    q = fmaf(d, d, q);
                }
            // the lane that holds the row's other 4-column groups (lk): both lanes end with the same pair of numbers
            const float mo = __shfl_xor(ml, 32), qo = __shfl_xor(q, 32), dm = ml - mo;
            mu[i] = 0.5f * (ml + mo);
            m2[i] = fmaf(dm * dm, 0.5f * kCnt, q + qo);
        }
        float2* sst = reinterpret_cast<float2*>(p_smem);          // [wc][128 rows]; the ring is idle once everybody is past its last fragment read
        float4* sgb = reinterpret_cast<float4*>(p_smem + 2048);   // gamma, beta of the tile's BN columns: read from LDS in the store loop (64 registers otherwise)
        __syncthreads();
        if (tid < BN / 2) sgb[tid] = *reinterpret_cast<const float4*>((tid < BN / 4 ? g.gamma + n0 + 4 * tid : g.beta + n0 + 4 * (tid - BN / 4)));
        if (lk == 0) {
#pragma unroll
            for (int i = 0; i < 2; ++i) sst[wc * 128 + wr * 64 + 32 * i + lr] = make_float2(mu[i], m2[i]);
        }
        __syncthreads();
        // The exchange runs on device-scope ATOMICS only (entries swapped in, the counter, entries read back) and no fence: an agent-scope
        // release / acquire fence writes back / invalidates the XCD's whole L2 -- with every workgroup's output rows dirty in it (measured:
        // 250 us per launch).  An entry's swap has RETURNED before its workgroup's barrier, the barrier precedes the count, and whoever
        // has seen the full count reads the entries with atomic loads.
        unsigned long long* st64 = reinterpret_cast<unsigned long long*>(g.ln_stats);
        if (tid < 128 && m0 + tid < g.M) {
            const float2 a = sst[tid], b = sst[128 + tid];
            const float dm = a.x - b.x;
            const float mean_t = 0.5f * (a.x + b.x), m2_t = fmaf(dm * dm, (float)kCnt, a.y + b.y);
            const unsigned long long pk = (unsigned long long)__builtin_bit_cast(uint32_t, mean_t) | ((unsigned long long)__builtin_bit_cast(uint32_t, m2_t) << 32);
            const unsigned long long was = __hip_atomic_exchange(st64 + (size_t)(m0 + tid) * kGX + bx, pk, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            asm volatile("" ::"v"(was));
        }
        __syncthreads();
        // MEMORY MODEL: relaxed agent-scope atomics order nothing but themselves; that the entries are visible to whoever sees the full count
        // rests on (a) the swap being a RETURNING atomic performed at the L2 / memory side, complete before the barrier that precedes the count,
        // and (b) the readers using atomic loads, which bypass the non-coherent per-CU / per-XCD caches -- how gfx950 executes device-scope
        // atomics as measured, NOT something the HIP memory model promises for relaxed order.  A port to another part re-derives this.
        // FORWARD PROGRESS: a waiting tile needs its row block's other column tiles resident or next in line (launch_gemm_p_ln_bn: whole row
        // blocks per XCD, in dispatch order; ln_fused_supported() gates the form on the part this was measured on).  The wait is BOUNDED: after
        // kLnWaitTicks of the 100 MHz clock (or as soon as any workgroup of the process has given up) the tile sets g_bert_status and goes on
        // with whatever it reads -- the forward's output is then invalid, the host reads the word (aspire_bert_status) and runs that forward
        // again with the separate layernorm_kernel pass.
        if (tid == 0) {
            if (!((g.probe & 16) && bx == 0))          // probe 16 (tests): the row block's first tile never counts itself -- its partners time out
                __hip_atomic_fetch_add(g.ln_count + by, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (!(g.probe & 8)) {
                const uint64_t t0 = __builtin_amdgcn_s_memrealtime();
                while (__hip_atomic_load(g.ln_count + by, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < kGX) {
                    __builtin_amdgcn_s_sleep(4);
                    if (__builtin_amdgcn_s_memrealtime() - t0 > kLnWaitTicks ||
                        (__hip_atomic_load(&g_bert_status, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & ASPIRE_BERT_STATUS_LN_TIMEOUT)) {
                        __hip_atomic_fetch_or(&g_bert_status, ASPIRE_BERT_STATUS_LN_TIMEOUT, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        break;
                    }
                }
            }
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int m = m0 + wr * 64 + 32 * i + lr;
            unsigned long long* srow = st64 + (size_t)min(m, g.M - 1) * kGX;
            float mt[kGX], qt[kGX];
#pragma unroll
            for (int t = 0; t < kGX; ++t) {
                const unsigned long long w = __hip_atomic_load(srow + t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                mt[t] = __builtin_bit_cast(float, (uint32_t)w);
                qt[t] = __builtin_bit_cast(float, (uint32_t)(w >> 32));
            }
            float sm = 0.f, sq = 0.f, sd = 0.f;
#pragma unroll
            for (int t = 0; t < kGX; ++t) sm += mt[t], sq += qt[t];
            const float mean = sm * (1.0f / kGX);
#pragma unroll
            for (int t = 0; t < kGX; ++t) sd = fmaf(mt[t] - mean, mt[t] - mean, sd);
            const float rstd = 1.0f / sqrtf(fmaf(sd, (float)BN, sq) * (1.0f / kD) + g.eps);
            if (m >= g.M) continue;
            float* crow = g.C ? g.C + (size_t)m * g.ldc + n0 + wc * 32 * TN + 8 * lk : nullptr;
#pragma unroll
            for (int j = 0; j < TN; ++j)
#pragma unroll
                for (int t = 0; t < 2; ++t) {
                    const int c4 = (wc * 32 * TN + 32 * j + 16 * t + 8 * lk) >> 2;
                    const float4 g0 = sgb[c4], g1 = sgb[c4 + 1], b0 = sgb[BN / 4 + c4], b1 = sgb[BN / 4 + c4 + 1];
                    const float g8[8] = {g0.x, g0.y, g0.z, g0.w, g1.x, g1.y, g1.z, g1.w}, b8[8] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
                    float o[8];
#pragma unroll
                    for (int c = 0; c < 8; ++c) o[c] = (acc[i][j][8 * t + c] - mean) * rstd * g8[c] + b8[c];
                    if (crow) {
                        *reinterpret_cast<float4*>(crow + 32 * j + 16 * t) = make_float4(o[0], o[1], o[2], o[3]);
                        *reinterpret_cast<float4*>(crow + 32 * j + 16 * t + 4) = make_float4(o[4], o[5], o[6], o[7]);
                    }
                    if (g.Cp) p_store8_at(g.Cp, p_slot8((uint32_t)g.M, (uint32_t)m, (uint32_t)(n0 + wc * 32 * TN + 32 * j + 16 * t + 8 * lk)), o);
                }
        }
    } else if constexpr (!SWAP) {
        // C/D layout of the 32 x 32 MFMA: col = lane & 31 (n), row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5) (m): a store instruction
        // writes two full 128-byte lines.  Whole tiles (all but the last row of tiles) take the branch-free form: the residual's 16
        // loads of a block go out together, the 16 stores follow back to back (with per-element row checks the compiler put an
        // s_waitcnt vmcnt(0) in front of every element: 64 serialised stores per wave, 4 us per workgroup on an idle chip and
        // 12 us when every CU stores at once -- 32 of the 120 us of an 8192 x 2304 x 768 launch)
        const bool whole = m0 + BM <= g.M;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                const int n = n0 + wc * 32 * TN + 32 * j + lr;
                const float bv = bias_n[j];
                const int mb = m0 + wr * 64 + 32 * i + 4 * lk;
                if (whole) {
                    float* crow = g.C + (size_t)mb * g.ldc + n;
                    float v[16];
#pragma unroll
                    for (int r = 0; r < 16; ++r) v[r] = fmaf(acc[i][j][r], kUnscale, bv);
                    if (!PERSIST && g.res) {
                        const float* rrow = g.res + (size_t)mb * g.ldr + n;
                        float rv[16];
#pragma unroll
                        for (int r = 0; r < 16; ++r) rv[r] = rrow[(size_t)((r & 3) + 8 * (r >> 2)) * g.ldr];
#pragma unroll
                        for (int r = 0; r < 16; ++r) v[r] += rv[r];
                    }
#pragma unroll
                    for (int r = 0; r < 16; ++r) crow[(size_t)((r & 3) + 8 * (r >> 2)) * g.ldc] = v[r];
                    continue;
                }
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int m = mb + (r & 3) + 8 * (r >> 2);
                    if (m >= g.M) continue;
                    float v = fmaf(acc[i][j][r], kUnscale, bv);
                    if (!PERSIST && g.res) v += g.res[(size_t)m * g.ldr + n];
                    g.C[(size_t)m * g.ldc + n] = v;
                }
            }
    } else {
        // swapped: col = lane & 31 is the row m, the registers run along n in groups of 4 consecutive: GELU(acc + bias) goes
        // straight into the P layout [M, N] (k dimension = n) of the next GEMM's A operand
        // (the bias vectors were fetched before the first store: a load between stores makes the compiler wait for every store
        // issued so far -- vmcnt counts both)
        // GELU in the accumulators' own layout (the bias vectors were fetched for it), then the lane pair exchanges register groups
        // (v_permlane32_swap, as the LayerNorm epilogue does): a lane owns 8 consecutive columns = one whole 16-byte piece per plane
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int m = m0 + wr * 64 + 32 * i + lr;
#pragma unroll
            for (int j = 0; j < TN; ++j)
#pragma unroll
                for (int t = 0; t < 2; ++t) {
                    float o[8];
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const float4 ba = bias_m[j][2 * t], bb = bias_m[j][2 * t + 1];
                        const float b_a = e == 0 ? ba.x : e == 1 ? ba.y : e == 2 ? ba.z : ba.w, b_b = e == 0 ? bb.x : e == 1 ? bb.y : e == 2 ? bb.z : bb.w;
                        float fa = fmaf(acc[i][j][8 * t + e], kUnscale, b_a), fb = fmaf(acc[i][j][8 * t + 4 + e], kUnscale, b_b);
                        if constexpr (EPI == 0) fa = gelu_erf(fa), fb = gelu_erf(fb);
                        auto r = __builtin_amdgcn_permlane32_swap(__builtin_bit_cast(int, fa), __builtin_bit_cast(int, fb), false, false);
                        const int x0 = r[0], x1 = r[1];
                        o[e] = __builtin_bit_cast(float, x0);
                        o[4 + e] = __builtin_bit_cast(float, x1);
                    }
                    if constexpr (EPI == 1) {
                        // planes [plane][Q | K | V][head][M][64]: the lane's 8 columns are one 16-byte piece of its row in one head
                        const int n = n0 + wc * 32 * TN + 32 * j + 16 * t + 8 * lk;        // 0 .. 2303: n / 64 = 12 (Q | K | V) + head
                        if (m < g.M) {
                            f16x8_t hh, ll;
                            split8_f16(o, hh, ll);
                            unsigned char* dst = (unsigned char*)g.Xp + ((size_t)(n >> 6) * (size_t)g.M + (size_t)m) * 128 + 2 * (n & 63);
                            *reinterpret_cast<f16x8_t*>(dst) = hh;
                            *reinterpret_cast<f16x8_t*>(dst + (size_t)36 * (size_t)g.M * 128) = ll;
                        }
                    } else if (m < g.M) p_store8_at(g.Cp, p_slot8((uint32_t)g.M, (uint32_t)m, (uint32_t)(n0 + wc * 32 * TN + 32 * j + 16 * t + 8 * lk)), o);
                }
        }
    }
    G_STAMP(3, __builtin_amdgcn_s_memrealtime());
    if constexpr (!PERSIST) {
        break;
    } else {
        if (!has_next) break;
        tile_i += tile_stride;
        first_tile = false;
        a_src = a_nxt;
        b_src = b_nxt;
        const uint32_t L = tile_lo + tile_i;
        m0 = (int)(L / gx) * 128;
        n0 = g.n_off + (int)(L % gx) * BN;
        load_bias();
        for (int i = 0; i < 2; ++i)
            for (int j = 0; j < TN; ++j) acc[i][j] = f32x16{};      // (constant trip counts: unrolled without being asked)
    }
  }
}

template <int NS, int KS, int BN, bool SWAP, bool PERSIST = false>
__global__ void __launch_bounds__(256, 2) gemm_p_kernel(PGemmArgs g) {
    gemm_p_body<NS, KS, BN, SWAP, PERSIST, false>(g);
}
// the QKV projection for flash_attn_p_kernel (launch_gemm_p_qkv): swapped orientation, the epilogue writes the planes [plane][Q | K | V][head][M][64]
__global__ void __launch_bounds__(256, 3) gemm_p_qkv_kernel(PGemmArgs g) {
    gemm_p_body<3, 1, 128, true, false, false, 128, 1>(g);
}
// 256 x BN tiles on eight waves (launch_gemm_p: ASPIRE_HIP_GEMM_TILE=256)
template <int BN, bool SWAP>
__global__ void __launch_bounds__(512, 4) gemm_p_w8_kernel(PGemmArgs g) {       // (the second bound is waves per SIMD: two workgroups of eight waves per CU)
    gemm_p_body<3, 1, BN, SWAP, false, false, 256>(g);
}
// the LayerNorm-epilogue form: THREE workgroups per CU asked of the register allocator (168 registers), as the plain forms get by themselves
template <int BN>
__global__ void __launch_bounds__(256, 3) gemm_p_ln_kernel(PGemmArgs g) {
    gemm_p_body<3, 1, BN, true, false, true>(g);
}

// One wave per row of 768: lane holds 3 float4 (d = 4*lane + 256*c).
// yp (optional): the row also goes out in the P layout (rows = `rows`), the A operand of the GEMM that reads it
__device__ __forceinline__ void layernorm_row(float4 (&v)[3], const float* gamma, const float* beta, float eps,
                                              float* out, int lane, void* yp = nullptr, int64_t rows = 0, int64_t row = 0) {
    float s = 0.f;
#pragma unroll
    for (int c = 0; c < 3; ++c) s += (v[c].x + v[c].y) + (v[c].z + v[c].w);
    const float mean = wave_sum(s) * (1.0f / kD);
    float q = 0.f;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float a = v[c].x - mean, b = v[c].y - mean, cc = v[c].z - mean, d = v[c].w - mean;
        q += (a * a + b * b) + (cc * cc + d * d);
    }
    const float rstd = 1.0f / sqrtf(wave_sum(q) * (1.0f / kD) + eps);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const int d = 4 * lane + 256 * c;
        const float4 gm = *reinterpret_cast<const float4*>(gamma + d), bt = *reinterpret_cast<const float4*>(beta + d);
        float4 o;
        o.x = (v[c].x - mean) * rstd * gm.x + bt.x;
        o.y = (v[c].y - mean) * rstd * gm.y + bt.y;
        o.z = (v[c].z - mean) * rstd * gm.z + bt.z;
        o.w = (v[c].w - mean) * rstd * gm.w + bt.w;
        *reinterpret_cast<float4*>(out + d) = o;
        if (yp) p_store4(yp, rows, row, d, o.x, o.y, o.z, o.w);
    }
}

__global__ void __launch_bounds__(256) layernorm_kernel(const float* __restrict__ x, const float* __restrict__ gamma,
                                                        const float* __restrict__ beta, float eps, float* __restrict__ y,
                                                        int64_t rows, void* __restrict__ yp) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    float4 v[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c] = *reinterpret_cast<const float4*>(x + row * kD + 4 * lane + 256 * c);
    layernorm_row(v, gamma, beta, eps, y + row * kD, lane, yp, rows, row);
}

__global__ void __launch_bounds__(256) embed_layernorm_kernel(const int64_t* __restrict__ tok, const int64_t* __restrict__ typ,
                                                              const float* __restrict__ word, const float* __restrict__ pos,
                                                              const float* __restrict__ type_emb, const float* __restrict__ gamma,
                                                              const float* __restrict__ beta, float eps, float* __restrict__ y,
                                                              int64_t rows, int64_t L, void* __restrict__ yp) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int64_t t = tok[row], ty = typ ? typ[row] : 0, p = row % L;
    float4 v[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const int d = 4 * lane + 256 * c;
        const float4 a = *reinterpret_cast<const float4*>(word + t * kD + d);
        const float4 b = *reinterpret_cast<const float4*>(type_emb + ty * kD + d);
        const float4 e = *reinterpret_cast<const float4*>(pos + p * kD + d);
        // BertEmbeddings: inputs_embeds + token_type_embeddings, then + position_embeddings
        v[c] = make_float4((a.x + b.x) + e.x, (a.y + b.y) + e.y, (a.z + b.z) + e.z, (a.w + b.w) + e.w);
    }
    layernorm_row(v, gamma, beta, eps, y + row * kD, lane, yp, rows, row);
}

// scores [rows = B*H*L][ld] in place: softmax_j(x_j * scale + (mask[b][j] ? 0 : -FLT_MAX)); columns in [L, ld)
// are written as zeros so that the P.V GEMM can run K up to ld.
__global__ void __launch_bounds__(256) softmax_mask_kernel(float* __restrict__ s, const int64_t* __restrict__ mask, int64_t rows,
                                                           int L, int ld, int rows_per_doc, float scale) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int64_t b = row / rows_per_doc;
    float* p = s + row * ld;
    const int64_t* mk = mask + b * L;
    constexpr int kMaxPer = 8;  // L <= 512
    float v[kMaxPer];
    float m = -INFINITY;
#pragma unroll
    for (int c = 0; c < kMaxPer; ++c) {
        const int j = lane + 64 * c;
        if (j < L) {
            // (1 - mask) * finfo(float32).min added to the scaled scores, as BertModel's extended mask
            v[c] = p[j] * scale + (mk[j] != 0 ? 0.f : -3.4028234663852886e38f);
            m = fmaxf(m, v[c]);
        } else {
            v[c] = -INFINITY;
        }
    }
    m = wave_max(m);
    float sum = 0.f;
#pragma unroll
    for (int c = 0; c < kMaxPer; ++c) {
        v[c] = (lane + 64 * c < L) ? expf(v[c] - m) : 0.f;
        sum += v[c];
    }
    const float inv = 1.0f / wave_sum(sum);
#pragma unroll
    for (int c = 0; c < kMaxPer; ++c) {
        const int j = lane + 64 * c;
        if (j < ld) p[j] = v[c] * inv;
    }
}

// ---------------------------------------------------------------------------------------------------------------
// Fused attention for one (document, head, 128 queries): softmax(Q K^T / 8 + mask) V without the [L, L] score
// matrix ever leaving the chip (the three-kernel form writes it, reads and rewrites it in the softmax, and reads it
// again: 400 MB per layer at B = 32, L = 256).  Everything is computed TRANSPOSED so that probabilities never change
// layout between the two products:
//   S^T = K Q^T   : keys are the MFMA M side, queries the N side -> in the 32x32 C layout lane n = lane & 31 is a
//                   QUERY and its 16 accumulator registers (x 4 row blocks) are KEYS.  The soft-max over keys is
//                   therefore in-register per lane, plus ONE exchange with lane ^ 32 (the other half of the keys).
//   O^T = V^T P^T : P^T is the B operand [k = key][n = query] -- lane n = query again, and the MFMA's k pair is
//                   (lanes < 32, lanes >= 32) = exactly the two key halves the C layout left in those lanes.  So
//                   accumulator register t of S^T goes straight back in as the B operand of step t.
// A wave owns 32 queries (their Q rows live in 32 registers for the whole kernel) and all keys; the 4 waves of a
// workgroup share the K tile (staged k-major, dims paired (d, d+8) so the half-waves read opposite LDS bank
// halves) and the V tile (row-major, 72-float rows: keys 4 apart land 32 banks apart).  Keys are walked in
// tiles of 128 with the usual running max / sum rescaling (flash attention), all in fp32 with exp2.
// HF semantics kept: scores / sqrt(64) + (1 - mask) * finfo.min, soft-max over keys (modeling_bert.py).
// ---------------------------------------------------------------------------------------------------------------
constexpr int kFaLdK = 132, kFaLdV = 72;
// ctxp (optional, instead of ctx): the context rows go out in the P layout [rows, 768] -- the A operand of the output projection
__global__ void __launch_bounds__(256, 2) flash_attn_f32_kernel(const float* __restrict__ qkv, const int64_t* __restrict__ mask,
                                                                float* __restrict__ ctx, int L, int H, void* __restrict__ ctxp,
                                                                int64_t rows) {
    __shared__ __attribute__((aligned(16))) float Ks[64][kFaLdK];     // [dim][key]
    __shared__ __attribute__((aligned(16))) float Vs[128][kFaLdV];    // [key][dim]
    __shared__ float kbias[128];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lr = lane & 31, lk = lane >> 5;
    const int qblocks = (L + 127) / 128;
    const int qb = blockIdx.x % qblocks, h = (blockIdx.x / qblocks) % H, b = blockIdx.x / (qblocks * H);
    const size_t ld = 3 * kD;
    const float* base = qkv + (size_t)b * L * ld + h * 64;
    const int q_row = qb * 128 + wave * 32 + lr;                      // this lane's query
    const bool q_ok = q_row < L;
    // Q^T operand registers: step t = 8 G + j multiplies dims (16 G + j | 16 G + 8 + j) in lanes (< 32 | >= 32)
    float qreg[32];
    {
        const float* qp = base + (size_t)min(q_row, L - 1) * ld;
#pragma unroll
        for (int G = 0; G < 4; ++G) {
            const float4 u = *reinterpret_cast<const float4*>(qp + 16 * G + 8 * lk);
            const float4 v = *reinterpret_cast<const float4*>(qp + 16 * G + 8 * lk + 4);
            qreg[8 * G + 0] = u.x; qreg[8 * G + 1] = u.y; qreg[8 * G + 2] = u.z; qreg[8 * G + 3] = u.w;
            qreg[8 * G + 4] = v.x; qreg[8 * G + 5] = v.y; qreg[8 * G + 6] = v.z; qreg[8 * G + 7] = v.w;
        }
    }
    f32x16 o[2];
#pragma unroll
    for (int mb = 0; mb < 2; ++mb)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[mb][r] = 0.f;
    float m_run = -INFINITY, l_run = 0.f;                              // l_run: this half-wave's share of the sum
    constexpr float kScaleLog2 = 0.125f * 1.44269504088896340736f;     // 1/sqrt(64) folded with log2(e)

    for (int k0 = 0; k0 < L; k0 += 128) {
        __syncthreads();                                               // previous tile fully consumed
        // ---- stage K (transposed) and V: thread -> key tid >> 1, 32 dims (tid & 1) * 32 .. -------------------
        {
            const int key = tid >> 1, d0 = (tid & 1) * 32;
            const bool ok = k0 + key < L;
            const float* kp = base + kD + (size_t)min(k0 + key, L - 1) * ld + d0;
            const float* vp = kp + kD;
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                float4 kv = *reinterpret_cast<const float4*>(kp + 4 * c);
                float4 vv = *reinterpret_cast<const float4*>(vp + 4 * c);
                if (!ok) kv = vv = make_float4(0.f, 0.f, 0.f, 0.f);
                Ks[d0 + 4 * c + 0][key] = kv.x;
                Ks[d0 + 4 * c + 1][key] = kv.y;
                Ks[d0 + 4 * c + 2][key] = kv.z;
                Ks[d0 + 4 * c + 3][key] = kv.w;
                *reinterpret_cast<float4*>(&Vs[key][d0 + 4 * c]) = vv;
            }
            if (tid < 128) {
                const int kk = k0 + tid;
                // additive mask in log2 units; keys past L are tile padding and must weigh exactly 0
                kbias[tid] = kk >= L ? -INFINITY : (mask[(size_t)b * L + kk] != 0 ? 0.f : -3.4028234663852886e38f);
            }
        }
        __syncthreads();
        // ---- S^T tile: 4 blocks of 32 keys x this wave's 32 queries -------------------------------------------
        f32x16 sacc[4];
#pragma unroll
        for (int rb = 0; rb < 4; ++rb)
#pragma unroll
            for (int r = 0; r < 16; ++r) sacc[rb][r] = 0.f;
#pragma unroll
        for (int t = 0; t < 32; ++t) {
            const int d = 16 * (t >> 3) + (t & 7) + 8 * lk;
#pragma unroll
            for (int rb = 0; rb < 4; ++rb)
                sacc[rb] = __builtin_amdgcn_mfma_f32_32x32x2f32(Ks[d][32 * rb + lr], qreg[t], sacc[rb], 0, 0, 0);
        }
        // ---- online soft-max over this tile's keys (registers of this lane + the other half-wave) -------------
        float tmax = -INFINITY;
#pragma unroll
        for (int rb = 0; rb < 4; ++rb)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int key = 32 * rb + 8 * (r >> 2) + 4 * lk + (r & 3);
                // scores * (1/8) + mask, then to log2 units; the mask constant times log2(e) overflows to -inf, which
                // exp2 maps to the same 0 that exp(-3.4e38 - max) gives
                sacc[rb][r] = fmaf(sacc[rb][r], kScaleLog2, kbias[key] * 1.44269504088896340736f);
                tmax = fmaxf(tmax, sacc[rb][r]);
            }
        tmax = fmaxf(tmax, lane_xor<32>(tmax));
        const float m_new = fmaxf(m_run, tmax);
        const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);     // exp2(-inf) = 0 on the first tile
        float psum = 0.f;
#pragma unroll
        for (int rb = 0; rb < 4; ++rb)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                sacc[rb][r] = __builtin_amdgcn_exp2f(sacc[rb][r] - m_new);
                psum += sacc[rb][r];
            }
        l_run = fmaf(l_run, alpha, psum);
        m_run = m_new;
#pragma unroll
        for (int mb = 0; mb < 2; ++mb)
#pragma unroll
            for (int r = 0; r < 16; ++r) o[mb][r] *= alpha;
        // ---- O^T += V^T P^T: accumulator register t of S^T is the B operand of step t -------------------------
#pragma unroll
        for (int rb = 0; rb < 4; ++rb)
#pragma unroll
            for (int t = 0; t < 16; ++t) {
                const int key = 32 * rb + 8 * (t >> 2) + 4 * lk + (t & 3);
#pragma unroll
                for (int mb = 0; mb < 2; ++mb)
                    o[mb] = __builtin_amdgcn_mfma_f32_32x32x2f32(Vs[key][32 * mb + lr], sacc[rb][t], o[mb], 0, 0, 0);
            }
    }
    // ---- normalise and store: lane = query, registers = head dims (4 consecutive per group) --------------------
    const float l_tot = l_run + lane_xor<32>(l_run);
    const float inv = 1.0f / l_tot;
    if (q_ok && ctxp) {
#pragma unroll
        for (int mb = 0; mb < 2; ++mb)
#pragma unroll
            for (int g4 = 0; g4 < 4; ++g4)
                p_store4(ctxp, rows, (int64_t)b * L + q_row, h * 64 + 32 * mb + 8 * g4 + 4 * lk, o[mb][4 * g4 + 0] * inv,
                         o[mb][4 * g4 + 1] * inv, o[mb][4 * g4 + 2] * inv, o[mb][4 * g4 + 3] * inv);
    } else if (q_ok) {
        float* op = ctx + ((size_t)b * L + q_row) * kD + h * 64;
#pragma unroll
        for (int mb = 0; mb < 2; ++mb)
#pragma unroll
            for (int g4 = 0; g4 < 4; ++g4)
                *reinterpret_cast<float4*>(op + 32 * mb + 8 * g4 + 4 * lk) =
                    make_float4(o[mb][4 * g4 + 0] * inv, o[mb][4 * g4 + 1] * inv, o[mb][4 * g4 + 2] * inv, o[mb][4 * g4 + 3] * inv);
    }
}

// ---------------------------------------------------------------------------------------------------------------
// The same fused attention on the fp16 matrix pipe at fp32 accuracy: every operand (Q, K, V, and the probabilities)
// goes in as two fp16 planes h + l (module comment of the P-layout GEMM: 24 significant bits; Q / K / V are O(1), P is in
// [0, 1]), three v_mfma_f32_32x32x16_f16 per term, sums and the whole soft-max in fp32.  Per 128-key tile and wave that is
// 96 MFMAs of 32 cycles against 256 fp32-input MFMAs of 64: 3 072 matrix-pipe cycles instead of 16 384.
//   S^T = K Q^T  : A = K planes [key][64 dims] (128-byte rows, 16-byte pieces XORed with the key's bits 1..3: conflict-free
//                  ds_read_b128), B = this lane's query, split once into 4 k steps x (h, l) registers.
//   O^T = V^T P^T: the MFMA's 8 consecutive k of lane half lk must be KEYS.  The S^T accumulators of lane half lk hold, per
//                  16-key group, keys {4 lk .. 4 lk + 3} and {8 + 4 lk .. 8 + 4 lk + 3}: P^T goes back in straight from the
//                  registers (converted to h + l in place), and the V^T image is built to match -- [dim][key slot], slots of a
//                  16-key group ordered [0-3, 8-11, 4-7, 12-15], so that a lane's 8 keys are one 16-byte read (256-byte rows,
//                  pieces XORed with the dim's low 4 bits).  V is transposed while it is staged: a thread owns 4 consecutive
//                  keys x 8 dims and writes 8-byte runs of 4 keys.
// ---------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256, 2) flash_attn_f16x2_kernel(const float* __restrict__ qkv, const int64_t* __restrict__ mask,
                                                                  float* __restrict__ ctx, int L, int H, void* __restrict__ ctxp,
                                                                  int64_t rows) {
    __shared__ __attribute__((aligned(16))) unsigned char Kp[2][128 * 128];    // [plane][key][64 dims fp16]
    __shared__ __attribute__((aligned(16))) unsigned char Vp[2][64 * 256];     // [plane][dim][128 key slots fp16]
    __shared__ float kbias[128];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lr = lane & 31, lk = lane >> 5;
    const int qblocks = (L + 127) / 128;
    // XCD-aware order (as the GEMMs'): XCD x = workgroup id mod 8 takes a contiguous run of the (document, head, query block) sequence, so the
    // query blocks of one (document, head) -- which stage the same K and V -- share an L2
    uint32_t wl;
    {
        const uint32_t nb = gridDim.x, bid = blockIdx.x, x = bid & 7, q8 = nb >> 3, r8 = nb & 7;
        wl = x * q8 + (x < r8 ? x : r8) + (bid >> 3);
    }
    const int qb = wl % qblocks, h = (wl / qblocks) % H, b = wl / (qblocks * H);
    const size_t ld = 3 * kD;
    const float* base = qkv + (size_t)b * L * ld + h * 64;
    const int q_row = qb * 128 + wave * 32 + lr;                      // this lane's query
    const bool q_ok = q_row < L;
    f16x8_t qh[4], ql[4];                                              // k step ks: dims 16 ks + 8 lk .. + 7
    {
        const float* qp = base + (size_t)min(q_row, L - 1) * ld + 8 * lk;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            const float4 u = *reinterpret_cast<const float4*>(qp + 16 * ks), v = *reinterpret_cast<const float4*>(qp + 16 * ks + 4);
            const float x[8] = {u.x, u.y, u.z, u.w, v.x, v.y, v.z, v.w};
            split8_f16(x, qh[ks], ql[ks]);
        }
    }
    f32x16 o[2];
#pragma unroll
    for (int mb = 0; mb < 2; ++mb)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[mb][r] = 0.f;
    float m_run = -INFINITY, l_run = 0.f;                              // l_run: this half-wave's share of the sum
    constexpr float kScaleLog2 = 0.125f * 1.44269504088896340736f;     // 1/sqrt(64) folded with log2(e)
    // fragment addresses: K rows 32 rb + lr, piece (2 ks + lk) ^ ((row >> 1) & 7); V^T rows 32 mb + lr, piece (2 s16 + lk) ^ (row & 15)
    const uint32_t k_rd = lr * 128 + 16 * (lk ^ ((lr >> 1) & 7)), k_sw = 0;
    (void)k_sw;
    const uint32_t v_rd = lr * 256 + 16 * (lk ^ (lr & 15) ^ (2 * (lr >> 4)));      // piece ^ f(row), f(d) = (d & 15) ^ 2 (d >> 4): see the V^T store

    for (int k0 = 0; k0 < L; k0 += 128) {
        __syncthreads();                                               // previous tile fully consumed
        {
            // ---- K: thread -> key tid >> 1, 32 dims (tid & 1) * 32 ..: four 8-dim pieces per plane ----
            const int key = tid >> 1, d0 = (tid & 1) * 32;
            const bool ok = k0 + key < L;
            const float* kp = base + kD + (size_t)min(k0 + key, L - 1) * ld + d0;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                float4 u = *reinterpret_cast<const float4*>(kp + 8 * c), v = *reinterpret_cast<const float4*>(kp + 8 * c + 4);
                if (!ok) u = v = make_float4(0.f, 0.f, 0.f, 0.f);
                const float x[8] = {u.x, u.y, u.z, u.w, v.x, v.y, v.z, v.w};
                f16x8_t hh, ll;
                split8_f16(x, hh, ll);
                const uint32_t at = key * 128 + 16 * ((d0 / 8 + c) ^ ((key >> 1) & 7));
                *reinterpret_cast<f16x8_t*>(&Kp[0][at]) = hh;
                *reinterpret_cast<f16x8_t*>(&Kp[1][at]) = ll;
            }
            // ---- V transposed: thread -> keys 4 kg .. 4 kg + 3 (kg = tid >> 3), dims 8 dg .. 8 dg + 7 (dg = tid & 7) ----
            const int kg = tid >> 3, dg = tid & 7;
            float vv[4][8];
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) {
                const int vkey = k0 + 4 * kg + kk;
                const float* vp = base + 2 * kD + (size_t)min(vkey, L - 1) * ld + 8 * dg;
                float4 u = *reinterpret_cast<const float4*>(vp), v = *reinterpret_cast<const float4*>(vp + 4);
                if (vkey >= L) u = v = make_float4(0.f, 0.f, 0.f, 0.f);
                vv[kk][0] = u.x; vv[kk][1] = u.y; vv[kk][2] = u.z; vv[kk][3] = u.w;
                vv[kk][4] = v.x; vv[kk][5] = v.y; vv[kk][6] = v.z; vv[kk][7] = v.w;
            }
            const int sub = kg & 3, slot4 = sub == 1 ? 2 : sub == 2 ? 1 : sub;      // [0-3, 8-11, 4-7, 12-15] within a 16-key group
            const int piece = 2 * (kg >> 2) + (slot4 >> 1), half = slot4 & 1;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int d = 8 * dg + j;
                typedef _Float16 f16x4_t __attribute__((ext_vector_type(4)));
                f16x4_t hh, ll;
#pragma unroll
                for (int kk = 0; kk < 4; ++kk) {
                    const _Float16 t = (_Float16)vv[kk][j];
                    hh[kk] = t;
                    ll[kk] = (_Float16)(vv[kk][j] - (float)t);
                }
                // the 16-byte piece XORed with f(d) = (d & 15) ^ 2 (d >> 4): the rows are 256 B = all 64 banks apart, and a wave's
                // stores of one j go to rows d = 8 dg + j, dg = 0 .. 7 -- with d & 15 alone (round 3) only two different swizzles for
                // eight rows: every store was a 4-way bank conflict (round-5 counters: 3.1 M conflict cycles of 5.9 M LDS cycles)
                const uint32_t at = d * 256 + 16 * (piece ^ (d & 15) ^ (2 * (d >> 4))) + 8 * half;
                *reinterpret_cast<f16x4_t*>(&Vp[0][at]) = hh;
                *reinterpret_cast<f16x4_t*>(&Vp[1][at]) = ll;
            }
            if (tid < 128) {
                const int kk = k0 + tid;
                // additive mask; keys past L are tile padding and must weigh exactly 0
                kbias[tid] = kk >= L ? -INFINITY : (mask[(size_t)b * L + kk] != 0 ? 0.f : -3.4028234663852886e38f);
            }
        }
        __syncthreads();
        // ---- S^T tile: 4 blocks of 32 keys x this wave's 32 queries; per k step the products l.h, h.l, h.h ----
        f32x16 sacc[4];
#pragma unroll
        for (int rb = 0; rb < 4; ++rb)
#pragma unroll
            for (int r = 0; r < 16; ++r) sacc[rb][r] = 0.f;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks)
#pragma unroll
            for (int rb = 0; rb < 4; ++rb) {
                const uint32_t at = (k_rd + rb * 32 * 128) ^ (32 * ks);
                const f16x8_t kh = *reinterpret_cast<const f16x8_t*>(&Kp[0][at]), kl = *reinterpret_cast<const f16x8_t*>(&Kp[1][at]);
                sacc[rb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(kl, qh[ks], sacc[rb], 0, 0, 0);
                sacc[rb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(kh, ql[ks], sacc[rb], 0, 0, 0);
                sacc[rb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(kh, qh[ks], sacc[rb], 0, 0, 0);
            }
        // ---- online soft-max over this tile's keys (registers of this lane + the other half-wave) -------------
        float tmax = -INFINITY;
#pragma unroll
        for (int rb = 0; rb < 4; ++rb)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int key = 32 * rb + 8 * (r >> 2) + 4 * lk + (r & 3);
                sacc[rb][r] = fmaf(sacc[rb][r], kScaleLog2, kbias[key] * 1.44269504088896340736f);
                tmax = fmaxf(tmax, sacc[rb][r]);
            }
        tmax = fmaxf(tmax, lane_xor<32>(tmax));
        const float m_new = fmaxf(m_run, tmax);
        const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);     // exp2(-inf) = 0 on the first tile
        float psum = 0.f;
#pragma unroll
        for (int rb = 0; rb < 4; ++rb)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                sacc[rb][r] = __builtin_amdgcn_exp2f(sacc[rb][r] - m_new);
                psum += sacc[rb][r];
            }
        l_run = fmaf(l_run, alpha, psum);
        m_run = m_new;
#pragma unroll
        for (int mb = 0; mb < 2; ++mb)
#pragma unroll
            for (int r = 0; r < 16; ++r) o[mb][r] *= alpha;
        // ---- O^T += V^T P^T: registers 8 g .. 8 g + 7 of S^T block rb are the 8 keys of k step 2 rb + g in this lane half ----
#pragma unroll
        for (int rb = 0; rb < 4; ++rb)
#pragma unroll
            for (int g2 = 0; g2 < 2; ++g2) {
                const float pv[8] = {sacc[rb][8 * g2 + 0], sacc[rb][8 * g2 + 1], sacc[rb][8 * g2 + 2], sacc[rb][8 * g2 + 3],
                                     sacc[rb][8 * g2 + 4], sacc[rb][8 * g2 + 5], sacc[rb][8 * g2 + 6], sacc[rb][8 * g2 + 7]};
                f16x8_t ph, pl;
                split8_f16(pv, ph, pl);
                const int s16 = 2 * rb + g2;
#pragma unroll
                for (int mb = 0; mb < 2; ++mb) {
                    const uint32_t at = (v_rd + mb * 32 * 256) ^ (32 * s16) ^ (64 * mb);      // (row >> 4 = 2 mb + (lr >> 4))
                    const f16x8_t vh = *reinterpret_cast<const f16x8_t*>(&Vp[0][at]), vl = *reinterpret_cast<const f16x8_t*>(&Vp[1][at]);
                    o[mb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vl, ph, o[mb], 0, 0, 0);
                    o[mb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vh, pl, o[mb], 0, 0, 0);
                    o[mb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vh, ph, o[mb], 0, 0, 0);
                }
            }
    }
    // ---- normalise and store: lane = query, registers = head dims (4 consecutive per group) --------------------
    const float l_tot = l_run + lane_xor<32>(l_run);
    const float inv = 1.0f / l_tot;
    if (ctxp) {
        // the lane pair exchanges register groups (v_permlane32_swap, as the GEMM epilogues do): a lane owns dims 16 t + 8 lk .. + 7 of a
        // 32-dim block = one whole 16-byte piece per plane (8-byte stores before)
#pragma unroll
        for (int mb = 0; mb < 2; ++mb)
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                float x[8];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float fa = o[mb][8 * t + e] * inv, fb = o[mb][8 * t + 4 + e] * inv;
                    auto r = __builtin_amdgcn_permlane32_swap(__builtin_bit_cast(int, fa), __builtin_bit_cast(int, fb), false, false);
                    const int x0 = r[0], x1 = r[1];
                    x[e] = __builtin_bit_cast(float, x0);
                    x[4 + e] = __builtin_bit_cast(float, x1);
                }
                if (q_ok) p_store8_at(ctxp, p_slot8((uint32_t)rows, (uint32_t)(b * L + q_row), (uint32_t)(h * 64 + 32 * mb + 16 * t + 8 * lk)), x);
            }
    } else if (q_ok) {
        float* op = ctx + ((size_t)b * L + q_row) * kD + h * 64;
#pragma unroll
        for (int mb = 0; mb < 2; ++mb)
#pragma unroll
            for (int g4 = 0; g4 < 4; ++g4)
                *reinterpret_cast<float4*>(op + 32 * mb + 8 * g4 + 4 * lk) =
                    make_float4(o[mb][4 * g4 + 0] * inv, o[mb][4 * g4 + 1] * inv, o[mb][4 * g4 + 2] * inv, o[mb][4 * g4 + 3] * inv);
    }
}

// ---------------------------------------------------------------------------------------------------------------
// Round 6: the same attention on operands the QKV GEMM has ALREADY split (launch_gemm_p_qkv): nothing is converted here but
// the probabilities, and the K / V tiles come into LDS by LDS-DMA -- asynchronously, a whole phase ahead -- instead of through
// global loads -> 300 VALU conversions per thread and tile -> ds_write (round-5 counters: VALU issue 9.7 k of a wave's 37 k
// cycles, the matrix pipe 6.1 k, 45 % of the wave cycles parked at waits behind the synchronous staging).
//   qkvp  fp16 [plane h | l][Q | K | V][head][M rows][64 dims]   (128-byte rows: one DMA instruction = 8 keys = 1 KB contiguous)
// V stays ROW-MAJOR in LDS ([key][64 dims], as K); the V^T fragments of O^T += V^T P^T come out of it through the LDS transpose
// read ds_read_b64_tr_b16: the 16 lanes of a group hand in four rows of 16 dims (lane i: row i >> 2, dims 4 (i & 3) .. + 3) and
// lane i receives dim i of the four rows (tools/ubench/trread.hip prints the mapping) -- the rows may be ANY four keys, so a lane
// half takes exactly the keys its S^T accumulators hold ({4 lk .. + 3} and {8 + 4 lk .. + 3} of a 16-key group) and P^T goes back
// in from the registers as before; no transposed image, no transposing store anywhere.
// Key tiles, planes and every sum are those of flash_attn_f16x2_kernel: the same bits.  Rows of a tile beyond the document are the
// next document's (or row M - 1 again): finite, weighted exactly 0.
// Schedule of a tile t (two barriers, as before): [K(t) landed, barrier X] issue V(t) DMA, key biases, S^T(t) [V(t) landed,
// barrier Y] issue K(t + 1) DMA, soft-max, O^T += V^T P^T.  Every DMA batch has a whole compute phase to land in.
// ---------------------------------------------------------------------------------------------------------------
// one LDS-DMA instruction: lane i moves 16 bytes from [sbase + voff(i)] to LDS [lds_dst + 16 i]  (M0 saved / restored: compiler-reserved)
__device__ __forceinline__ void glds16(uint64_t sbase, uint32_t voff, uint32_t lds_dst) {
    uint32_t keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\t"
                 "global_load_lds_dwordx4 %1, %2\n\t"
                 "s_mov_b32 m0, %0"
                 : "=&s"(keep)
                 : "v"(voff), "s"(sbase), "s"(lds_dst)
                 : "memory");
}
// four keys x 16 dims, transposed: see above
typedef __fp16 fp16x4_raw __attribute__((__vector_size__(4 * sizeof(__fp16))));
__device__ __forceinline__ f16x8_t lds_tr_pair(const unsigned char* a0, const unsigned char* a1) {
    typedef _Float16 h4 __attribute__((ext_vector_type(4)));
    const fp16x4_raw x = __builtin_amdgcn_ds_read_tr16_b64_v4f16((__attribute__((address_space(3))) fp16x4_raw*)a0);
    const fp16x4_raw y = __builtin_amdgcn_ds_read_tr16_b64_v4f16((__attribute__((address_space(3))) fp16x4_raw*)a1);
    const h4 xh = __builtin_bit_cast(h4, x), yh = __builtin_bit_cast(h4, y);
    return __builtin_shufflevector(xh, yh, 0, 1, 2, 3, 4, 5, 6, 7);
}

// KT = keys per tile: 128 (two workgroups per CU: 66 KB of LDS each) or 64 (ASPIRE_HIP_ATTN=p64: 33 KB and 32 accumulator registers fewer -- three per CU;
// other tile edges, so other online-soft-max groupings: equal to the 128-key form to rounding, not bit for bit)
template <int KT>
__device__ __forceinline__ void flash_attn_p_body(const unsigned char* __restrict__ qkvp, const int64_t* __restrict__ mask,
                                                  float* __restrict__ ctx, int L, int H, void* __restrict__ ctxp, int64_t rows) {
    constexpr int NRB = KT / 32;                                               // 32-key blocks per tile
    __shared__ __attribute__((aligned(16))) unsigned char Kp[2][KT * 128];    // [plane][key][64 dims fp16], piece ^ ((key >> 1) & 7)
    __shared__ __attribute__((aligned(16))) unsigned char Vp[2][KT * 128];    // [plane][key][64 dims fp16], piece ^ 4 ((key >> 1) & 1)
    __shared__ float kbias[KT];
    const int tid = threadIdx.x, lane = tid & 63, lr = lane & 31, lk = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int qblocks = (L + 127) / 128;
    uint32_t wl;
    {
        const uint32_t nb = gridDim.x, bid = blockIdx.x, x = bid & 7, q8 = nb >> 3, r8 = nb & 7;
        wl = x * q8 + (x < r8 ? x : r8) + (bid >> 3);
    }
    const int qb = wl % qblocks, h = (wl / qblocks) % H, b = wl / (qblocks * H);
    const int64_t doc0 = (int64_t)b * L;                               // first row of the document
    const int q_row = qb * 128 + wave * 32 + lr;                       // this lane's query
    const bool q_ok = q_row < L;
    const size_t plane_b = (size_t)3 * H * rows * 128;                 // bytes of one plane
    f16x8_t qh[4], ql[4];                                              // k step ks: dims 16 ks + 8 lk .. + 7 = piece 2 ks + lk of the row
    {
        const unsigned char* qp = qkvp + ((size_t)h * rows + (size_t)(doc0 + min(q_row, L - 1))) * 128 + 16 * lk;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            qh[ks] = *reinterpret_cast<const f16x8_t*>(qp + 32 * ks);
            ql[ks] = *reinterpret_cast<const f16x8_t*>(qp + plane_b + 32 * ks);
        }
    }
    f32x16 o[2];
#pragma unroll
    for (int mb = 0; mb < 2; ++mb)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[mb][r] = 0.f;
    float m_run = -INFINITY, l_run = 0.f;
    constexpr float kScaleLog2 = 0.125f * 1.44269504088896340736f;
    const uint32_t k_rd = lr * 128 + 16 * (lk ^ ((lr >> 1) & 7));
    // V transpose read: lane = (lk, dim half dh, i): hands in row 4 lk + (i >> 2) (+ 8 for the second read) of a 16-key group, dims 32 mb + 16 dh + 4 (i & 3) ..:
    // piece 4 mb + 2 dh + ((i & 3) >> 1), byte 8 (i & 1) in it; the piece is XORed with 4 ((key >> 1) & 1) = 4 ((i >> 3) & 1): keys two apart, 256 B
    // apart in the image, sit in different halves of the bank row
    const int vi = lane & 15, vdh = (lane >> 4) & 1;
    const uint32_t v_rd = (4 * lk + (vi >> 2)) * 128 + 16 * ((2 * vdh + ((vi & 3) >> 1)) ^ (4 * ((vi >> 3) & 1))) + 8 * (vi & 1);
    const uint32_t lds_k = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) unsigned char*)&Kp[0][0];
    const uint32_t lds_v = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) unsigned char*)&Vp[0][0];
    const int n_tiles = (L + KT - 1) / KT;
    // wave w moves keys 32 w .. 32 w + 31 of both planes of K (and of V), 8 keys per instruction: lane i -> key 8 c + (i >> 3), LDS piece i & 7 =
    // the row's piece (i & 7) ^ swizzle(key)
    const uint64_t k_base = (uint64_t)(uintptr_t)qkvp + ((size_t)(H + h) * rows) * 128;
    const uint64_t v_base = (uint64_t)(uintptr_t)qkvp + ((size_t)(2 * H + h) * rows) * 128;
    auto issue_kv = [&](int t, bool is_v) {
        const int64_t g = doc0 + (int64_t)t * KT;
#pragma unroll
        for (int c = 0; c < KT / 32; ++c) {
            const int key = (KT / 4) * wave + 8 * c + (lane >> 3);
            const int64_t row = min(g + key, rows - 1);
            const int sw = is_v ? 4 * ((key >> 1) & 1) : (key >> 1) & 7;
            const uint32_t voff = (uint32_t)(row * 128) + 16 * ((lane & 7) ^ sw);      // (< 4 GB per head: launch_gemm_p_qkv checks)
#pragma unroll
            for (int pl = 0; pl < 2; ++pl)
                glds16((is_v ? v_base : k_base) + pl * plane_b, voff, (is_v ? lds_v : lds_k) + pl * (KT * 128) + ((KT / 4) * wave + 8 * c) * 128);
        }
    };

    issue_kv(0, false);
    for (int t = 0; t < n_tiles; ++t) {
        const int k0 = t * KT;
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");               // X: this wave's pieces of K(t) have landed ...
        __syncthreads();                                               // ... everybody's; and everybody is past PV(t - 1): the V image is free
        issue_kv(t, true);
        if (tid < KT) {
            const int kk = k0 + tid;
            // additive mask; keys past L are tile padding (the next document's rows) and must weigh exactly 0
            // (stored times log2(e), as the soft-max below wants it: the same product as flash_attn_f16x2_kernel forms per score)
            kbias[tid] = (kk >= L ? -INFINITY : (mask[(size_t)doc0 + kk] != 0 ? 0.f : -3.4028234663852886e38f)) * 1.44269504088896340736f;
        }
        // ---- S^T tile: 4 blocks of 32 keys x this wave's 32 queries; per k step the products l.h, h.l, h.h ----
        f32x16 sacc[NRB];
        const f32x16 zero16 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        // (consecutive MFMAs go to DIFFERENT accumulators -- the three products of a term run across the four key blocks -- so that none waits
        // for its predecessor's result; every accumulator still takes its products in the order l.h, h.l, h.h: the same sums)
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            f16x8_t kh[NRB], kl[NRB];
#pragma unroll
            for (int rb = 0; rb < NRB; ++rb) {
                const uint32_t at = (k_rd + rb * 32 * 128) ^ (32 * ks);
                kh[rb] = *reinterpret_cast<const f16x8_t*>(&Kp[0][at]);
                kl[rb] = *reinterpret_cast<const f16x8_t*>(&Kp[1][at]);
            }
#pragma unroll
            for (int rb = 0; rb < NRB; ++rb) sacc[rb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(kl[rb], qh[ks], ks == 0 ? zero16 : sacc[rb], 0, 0, 0);
#pragma unroll
            for (int rb = 0; rb < NRB; ++rb) sacc[rb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(kh[rb], ql[ks], sacc[rb], 0, 0, 0);
#pragma unroll
            for (int rb = 0; rb < NRB; ++rb) sacc[rb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(kh[rb], qh[ks], sacc[rb], 0, 0, 0);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");               // Y: this wave's pieces of V(t) have landed ...
        __syncthreads();                                               // ... everybody's, the key biases too; and everybody is past S^T(t): the K image is free
        if (t + 1 < n_tiles) issue_kv(t + 1, false);
        // ---- online soft-max over this tile's keys (registers of this lane + the other half-wave) -------------
        float tmax = -INFINITY;
#pragma unroll
        for (int rb = 0; rb < NRB; ++rb)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int key = 32 * rb + 8 * (r >> 2) + 4 * lk + (r & 3);
                sacc[rb][r] = fmaf(sacc[rb][r], kScaleLog2, kbias[key]);
                tmax = fmaxf(tmax, sacc[rb][r]);
            }
        tmax = fmaxf(tmax, lane_xor<32>(tmax));
        const float m_new = fmaxf(m_run, tmax);
        const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);     // exp2(-inf) = 0 on the first tile
        float psum = 0.f;
#pragma unroll
        for (int rb = 0; rb < NRB; ++rb)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                sacc[rb][r] = __builtin_amdgcn_exp2f(sacc[rb][r] - m_new);
                psum += sacc[rb][r];
            }
        l_run = fmaf(l_run, alpha, psum);
        m_run = m_new;
#pragma unroll
        for (int mb = 0; mb < 2; ++mb)
#pragma unroll
            for (int r = 0; r < 16; ++r) o[mb][r] *= alpha;
        // ---- O^T += V^T P^T: registers 8 g .. 8 g + 7 of S^T block rb are the 8 keys of k step 2 rb + g in this lane half: keys
        // 16 s16 + {4 lk .. + 3} and 16 s16 + 8 + {4 lk .. + 3} -- the two transpose reads of the V^T fragment take exactly those rows ----
#pragma unroll
        for (int rb = 0; rb < NRB; ++rb)
#pragma unroll
            for (int g2 = 0; g2 < 2; ++g2) {
                const float pv[8] = {sacc[rb][8 * g2 + 0], sacc[rb][8 * g2 + 1], sacc[rb][8 * g2 + 2], sacc[rb][8 * g2 + 3],
                                     sacc[rb][8 * g2 + 4], sacc[rb][8 * g2 + 5], sacc[rb][8 * g2 + 6], sacc[rb][8 * g2 + 7]};
                f16x8_t ph, pl;
                split8_f16(pv, ph, pl);
                const int s16 = 2 * rb + g2;
                f16x8_t vh[2], vl[2];
#pragma unroll
                for (int mb = 0; mb < 2; ++mb) {
                    // rows 16 s16 + 4 lk + (i >> 2) and + 8: (key >> 1) & 1 is the same for both ((i >> 3) & 1: 16 s16, 4 lk and 8 leave bit 1 alone);
                    // dims 32 mb ..: pieces 4 mb .. -> ^ (64 mb) on the byte offset
                    const uint32_t at = (v_rd + s16 * 16 * 128) ^ (64 * mb);
                    vh[mb] = lds_tr_pair(&Vp[0][at], &Vp[0][at + 8 * 128]);
                    vl[mb] = lds_tr_pair(&Vp[1][at], &Vp[1][at + 8 * 128]);
                }
                // (the two dim blocks alternate: no MFMA directly behind the one whose result it accumulates onto)
#pragma unroll
                for (int mb = 0; mb < 2; ++mb) o[mb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vl[mb], ph, o[mb], 0, 0, 0);
#pragma unroll
                for (int mb = 0; mb < 2; ++mb) o[mb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vh[mb], pl, o[mb], 0, 0, 0);
#pragma unroll
                for (int mb = 0; mb < 2; ++mb) o[mb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vh[mb], ph, o[mb], 0, 0, 0);
            }
    }
    // ---- normalise and store (as flash_attn_f16x2_kernel) --------------------------------------------------------
    const float l_tot = l_run + lane_xor<32>(l_run);
    const float inv = 1.0f / l_tot;
    if (ctxp) {
#pragma unroll
        for (int mb = 0; mb < 2; ++mb)
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                float x[8];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float fa = o[mb][8 * t + e] * inv, fb = o[mb][8 * t + 4 + e] * inv;
                    auto r = __builtin_amdgcn_permlane32_swap(__builtin_bit_cast(int, fa), __builtin_bit_cast(int, fb), false, false);
                    const int x0 = r[0], x1 = r[1];
                    x[e] = __builtin_bit_cast(float, x0);
                    x[4 + e] = __builtin_bit_cast(float, x1);
                }
                if (q_ok) p_store8_at(ctxp, p_slot8((uint32_t)rows, (uint32_t)(doc0 + q_row), (uint32_t)(h * 64 + 32 * mb + 16 * t + 8 * lk)), x);
            }
    } else if (q_ok) {
        float* op = ctx + ((size_t)doc0 + q_row) * kD + h * 64;
#pragma unroll
        for (int mb = 0; mb < 2; ++mb)
#pragma unroll
            for (int g4 = 0; g4 < 4; ++g4)
                *reinterpret_cast<float4*>(op + 32 * mb + 8 * g4 + 4 * lk) =
                    make_float4(o[mb][4 * g4 + 0] * inv, o[mb][4 * g4 + 1] * inv, o[mb][4 * g4 + 2] * inv, o[mb][4 * g4 + 3] * inv);
    }
}

__global__ void __launch_bounds__(256, 2) flash_attn_p_kernel(const unsigned char* __restrict__ qkvp, const int64_t* __restrict__ mask,
                                                              float* __restrict__ ctx, int L, int H, void* __restrict__ ctxp, int64_t rows) {
    flash_attn_p_body<128>(qkvp, mask, ctx, L, H, ctxp, rows);
}
#ifndef ASPIRE_ATTN64_WAVES      // (experiment builds: 2 = leave a third of the SIMD's registers to another stream's GEMM waves)
#define ASPIRE_ATTN64_WAVES 3
#endif
__global__ void __launch_bounds__(256, ASPIRE_ATTN64_WAVES) flash_attn_p64_kernel(const unsigned char* __restrict__ qkvp, const int64_t* __restrict__ mask,
                                                                float* __restrict__ ctx, int L, int H, void* __restrict__ ctxp, int64_t rows) {
    flash_attn_p_body<64>(qkvp, mask, ctx, L, H, ctxp, rows);
}

// fraction of the last round of workgroups that runs empty, at 3 resident workgroups per CU
double gemm_rounds_waste(long long blocks) {
    const double rounds = (double)blocks / 768.0;
    const double full = (double)((blocks + 767) / 768);
    return (full - rounds) / full;
}

template <bool B_KN>
int launch_gemm(const GemmArgs& g, int batch, hipStream_t st) {
    // Tile choice: the largest tile that still gives >= ~2 blocks per CU; small-N GEMMs (N = 768 on 8192 rows is
    // only 384 blocks of 128x128) drop to 128x64 / 64x64 to avoid a half-empty last wave of blocks.
    const long long b128 = (long long)((g.M + 127) / 128) * ((g.N + 127) / 128) * batch;
    const long long b12864 = (long long)((g.M + 127) / 128) * ((g.N + 63) / 64) * batch;
    // BK = 16 with double-buffered LDS (34 KB / block, 3 blocks per CU) measured 96 TFLOP/s end to end against
    // 85 for BK = 32 (67 KB, 2 blocks per CU): occupancy matters more than halving the barrier count here.
    // 96-column tiles (4 waves stacked on M, 32 x 96 each) when they divide N and fill whole rounds of the 768
    // resident workgroups where 128-column tiles leave half a round idle (QKV, N = 2304: 1152 -> 1536 workgroups).
    const long long b12896 = (long long)((g.M + 127) / 128) * (g.N / 96) * batch;
    const bool force96 = tuning().gemm_tile96 && g.N % 96 == 0;   // tuning only
    // nn.Linear shapes (both operands k-contiguous, K a multiple of the 16-wide bf16 MFMA step): the bf16x3 form.
    // Default for these shapes; 128 x 128 tiles wherever they give every CU a workgroup (measured at M = 8192: N = 768 149-175
    // TFLOP/s-equivalent against 136-151 with 128 x 64 tiles, N = 2304 166 against 148 with 128 x 96 -- the wider wave tile
    // reads less LDS per MFMA, and LDS bandwidth is what the six-product form runs into next).
    if constexpr (!B_KN) {
        if (tuning().gemm_form != 1 && g.K % 16 == 0) {       // (gemm_form 3 = planes pins the P layout in the forward; a bare GEMM has none)
            const int ft = tuning().gemm_tile;
            if (ft == 96 && g.N % 96 == 0) {
                hipLaunchKernelGGL((gemm_bf16x3_kernel<128, 96, 1>), dim3(g.N / 96, (g.M + 127) / 128, batch), dim3(256), 0, st, g);
            } else if (ft == 128 || (ft == 0 && b128 >= 256 && g.N >= 128)) {
                hipLaunchKernelGGL((gemm_bf16x3_kernel<128, 128>), dim3((g.N + 127) / 128, (g.M + 127) / 128, batch), dim3(256), 0, st, g);
            } else if (ft == 64 || (ft == 0 && b12864 >= 256)) {
                hipLaunchKernelGGL((gemm_bf16x3_kernel<128, 64>), dim3((g.N + 63) / 64, (g.M + 127) / 128, batch), dim3(256), 0, st, g);
            } else {
                hipLaunchKernelGGL((gemm_bf16x3_kernel<64, 64>), dim3((g.N + 63) / 64, (g.M + 63) / 64, batch), dim3(256), 0, st, g);
            }
            ASPIRE_LAUNCH_OK();
            return ASPIRE_OK;
        }
    }
    if (!B_KN && g.N % 96 == 0 && (force96 || (b12896 >= 768 && gemm_rounds_waste(b12896) + 0.05 < gemm_rounds_waste(b128)))) {
        dim3 grid(g.N / 96, (g.M + 127) / 128, batch);
        hipLaunchKernelGGL((gemm_f32_kernel<128, 96, 16, false, 1>), grid, dim3(256), 0, st, g);
    } else if (b128 >= 512 && g.N >= 128) {
        dim3 grid((g.N + 127) / 128, (g.M + 127) / 128, batch);
        hipLaunchKernelGGL((gemm_f32_kernel<128, 128, 16, B_KN>), grid, dim3(256), 0, st, g);
    } else if (b12864 >= 512) {
        dim3 grid((g.N + 63) / 64, (g.M + 127) / 128, batch);
        hipLaunchKernelGGL((gemm_f32_kernel<128, 64, 16, B_KN>), grid, dim3(256), 0, st, g);
    } else {
        dim3 grid((g.N + 63) / 64, (g.M + 63) / 64, batch);
        hipLaunchKernelGGL((gemm_f32_kernel<64, 64, 16, B_KN>), grid, dim3(256), 0, st, g);
    }
    ASPIRE_LAUNCH_OK();
    return ASPIRE_OK;
}

size_t align_up(size_t x) { return (x + 255) & ~(size_t)255; }

struct Workspace {
    float *x, *qkv, *scores, *ctx, *tmp, *ffn;
    void *actp, *ctxp, *ffnp;       // P-layout activations (pre-split GEMM operands): LayerNorm outputs, attention context, GELU(FFN1)
    float2* ln_stats;               // the LayerNorm-epilogue GEMMs' per-row, per-column-tile moments [M][12]
    int* ln_count;                  // their arrival counters [2 n_layers][row blocks], zeroed once per forward
    size_t ln_count_bytes;
    unsigned char* qkvp;            // round 6: the attention's operands as the QKV GEMM splits them (flash_attn_p_kernel): [plane][Q | K | V][head][M][64] fp16
    size_t total;
};

Workspace carve(void* base, int64_t B, int64_t L, int heads, int ffn_dim, int n_layers) {
    const size_t M = (size_t)B * L, Lp = (size_t)(L + 3) / 4 * 4;
    char* p = (char*)base;
    Workspace w;
    size_t off = 0;
    auto take = [&](size_t nfloats) {
        float* r = (float*)(p + off);
        off += align_up(nfloats * sizeof(float));
        return r;
    };
    w.x = take(M * kD);
    w.qkv = take(M * 3 * kD);
    w.scores = take((size_t)B * heads * L * Lp);
    w.ctx = take(M * kD);
    w.tmp = take(M * kD);
    w.ffn = take(M * ffn_dim);
    auto take_p = [&](int64_t K) {
        void* r = p + off;
        off += align_up(p_bytes((int64_t)M, K));
        return r;
    };
    w.actp = take_p(kD);
    w.ctxp = take_p(kD);
    w.ffnp = take_p(ffn_dim);
    w.ln_stats = reinterpret_cast<float2*>(take(M * 24));
    w.ln_count_bytes = (size_t)2 * (n_layers > 0 ? n_layers : 0) * ((M + 127) / 128) * sizeof(int);
    w.ln_count = reinterpret_cast<int*>(take(w.ln_count_bytes / sizeof(float) + 1));
    w.qkvp = reinterpret_cast<unsigned char*>(take(M * 3 * kD));                     // 2 planes x [Q | K | V] x M x 768 fp16 = the bytes of the fp32 qkv
    w.total = off;
    return w;
}

// Launch of the P-layout GEMM (N % 128 == 0, K % 16 == 0): 128 x 128 tiles (wider wave tile: less LDS traffic per MFMA), or
// 128 x 64 for a short-k GEMM whose 128-wide tiles could not give every resident workgroup slot a tile.  (Splitting the columns
// of a GEMM into a launch of 128-wide tiles filling whole rounds and a launch of 64-wide ones for the rest -- 8192 x 2304: 768 +
// 768 tiles instead of 1152 = 1.5 rounds -- was built and measured: 164 us either way.  A half-empty last round is not the
// loss it looks like: its workgroups run faster for having the CU's matrix pipes to themselves.)
// the persistent form of the default ring: 768 resident workgroups (three per CU) walk the tiles
template <int BN, bool SWAP>
int launch_gemm_p_persist(PGemmArgs g, int n_off, int col_tiles, hipStream_t st) {
    constexpr int NS = 3, lds = NS * (kPTile + BN * kPRowBytes);
    static hipError_t raised = hipFuncSetAttribute(reinterpret_cast<const void*>(gemm_p_kernel<NS, 1, BN, SWAP, true>),
                                                   hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    ASPIRE_HIP_OK(raised);
    g.n_off = n_off;
    g.probe = 0;
    g.tiles_x = col_tiles;
    g.tiles_y = (g.M + 127) / 128;
    const long long tiles = (long long)g.tiles_x * g.tiles_y;
    hipLaunchKernelGGL((gemm_p_kernel<NS, 1, BN, SWAP, true>), dim3((unsigned)(tiles < 768 ? tiles : 768)), dim3(256), lds, st, g);
    ASPIRE_LAUNCH_OK();
    return ASPIRE_OK;
}
template <int NS, int KS, int BN, bool SWAP>
int launch_gemm_p_ns(PGemmArgs g, int n_off, int col_tiles, hipStream_t st) {
    constexpr int lds = NS * KS * (kPTile + BN * kPRowBytes);
    static hipError_t raised = hipFuncSetAttribute(reinterpret_cast<const void*>(gemm_p_kernel<NS, KS, BN, SWAP>),
                                                   hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    ASPIRE_HIP_OK(raised);
    g.n_off = n_off;
    g.probe = tuning().gemm_probe;
    hipLaunchKernelGGL((gemm_p_kernel<NS, KS, BN, SWAP>), dim3(col_tiles, (g.M + 127) / 128), dim3(256), lds, st, g);
    ASPIRE_LAUNCH_OK();
    return ASPIRE_OK;
}
template <int BN, bool SWAP>
int launch_gemm_p_ring(const PGemmArgs& g, int n_off, int col_tiles, hipStream_t st) {
    // ASPIRE_HIP_GEMM_RING = 10 KS + NS pins the ring (default: kPRingDefault); 113: the default ring's persistent form
    if (tuning().gemm_ring == 113 && !g.res && g.bias && (g.K / 16) % 3 == 0 && (long long)col_tiles * ((g.M + 127) / 128) > 768)
        return launch_gemm_p_persist<BN, SWAP>(g, n_off, col_tiles, st);
    switch (tuning().gemm_ring ? tuning().gemm_ring % 100 : kPRingDefault) {
    case 12: return launch_gemm_p_ns<2, 1, BN, SWAP>(g, n_off, col_tiles, st);
    case 14: return launch_gemm_p_ns<4, 1, BN, SWAP>(g, n_off, col_tiles, st);
    case 23: return launch_gemm_p_ns<3, 2, BN, SWAP>(g, n_off, col_tiles, st);
    case 22: return launch_gemm_p_ns<2, 2, BN, SWAP>(g, n_off, col_tiles, st);
    default: return launch_gemm_p_ns<3, 1, BN, SWAP>(g, n_off, col_tiles, st);
    }
}
template <bool SWAP>
int launch_gemm_p_w8(PGemmArgs g, hipStream_t st) {
    constexpr int lds = 3 * (256 + 128) * kPRowBytes;
    static hipError_t raised = hipFuncSetAttribute(reinterpret_cast<const void*>(gemm_p_w8_kernel<128, SWAP>), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    ASPIRE_HIP_OK(raised);
    g.n_off = 0;
    g.probe = 0;
    hipLaunchKernelGGL((gemm_p_w8_kernel<128, SWAP>), dim3(g.N / 128, (g.M + 255) / 256), dim3(512), lds, st, g);
    ASPIRE_LAUNCH_OK();
    return ASPIRE_OK;
}
template <bool SWAP>
int launch_gemm_p(const PGemmArgs& g, hipStream_t st) {
    ASPIRE_REQUIRE(g.N % 128 == 0 && g.K % 32 == 0, ASPIRE_ERR_UNSUPPORTED, "P-layout GEMM needs N %% 128 == 0 and K %% 32 == 0");
    // 256 x 128 tiles on eight waves: pinned (ASPIRE_HIP_GEMM_TILE=256), and by default for the GELU GEMM (the one SWAP launch of a layer, N = 3072)
    // when its tiles fill the 512 slots of that form in whole rounds or many of them (64 x 256 tokens: 1536 tiles = 3 rounds)
    {
        const long long t8 = (long long)(g.N / 128) * ((g.M + 255) / 256);
        // (... and for the QKV GEMM when its tiles balance over the 256 CUs: 32 768 rows x 2304 columns = 2304 tiles, 9 per CU; at 16 384 rows
        // 1152 tiles are 4.5 per CU and the 128 x 128 form wins)
        if (tuning().gemm_tile == 256 || (tuning().gemm_tile == 0 && SWAP && (t8 % 512 == 0 || t8 >= 2048)) ||
            (tuning().gemm_tile == 0 && !SWAP && !g.res && g.N > kD && t8 % 256 == 0 && t8 >= 2048))
            return launch_gemm_p_w8<SWAP>(g, st);
    }
    const long long slots = 768, rows = (g.M + 127) / 128, n128 = g.N / 128;
    // 128 x 64 tiles (twice the workgroups) where 128 x 128 ones cannot give every workgroup slot a tile and the k loop is short
    int c1 = (int)n128;
    if (tuning().gemm_tile == 64 || (tuning().gemm_tile == 0 && rows * n128 < slots && g.K <= 1024)) c1 = 0;
    if (c1 > 0)
        if (int rc = launch_gemm_p_ring<128, SWAP>(g, 0, c1, st)) return rc;
    if (c1 < n128)
        if (int rc = launch_gemm_p_ring<64, SWAP>(g, c1 * 128, (int)(n128 - c1) * 2, st)) return rc;
    return ASPIRE_OK;
}
// The QKV projection for flash_attn_p_kernel: one launch of 18 column tiles in the swapped orientation (a lane owns 8 consecutive columns of its
// token row = one 16-byte piece per plane), the epilogue writes Q, K and V as fp16 planes per head.
int launch_gemm_p_qkv(PGemmArgs g, hipStream_t st) {
    constexpr int lds = 3 * (kPTile + 128 * kPRowBytes);
    static hipError_t raised = hipFuncSetAttribute(reinterpret_cast<const void*>(gemm_p_qkv_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    ASPIRE_HIP_OK(raised);
    ASPIRE_REQUIRE(g.N == 3 * kD && g.K == kD && g.bias && g.Xp, ASPIRE_ERR_INVALID_ARG, "QKV projection: [M, 768] x [2304, 768]^T + bias -> planes");
    ASPIRE_REQUIRE((uint64_t)g.M * 128 < (1ull << 32), ASPIRE_ERR_UNSUPPORTED, "%d token rows: the planes of a head are addressed in 32 bits", g.M);
    g.probe = 0;
    g.n_off = 0;
    hipLaunchKernelGGL(gemm_p_qkv_kernel, dim3(3 * kD / 128, (g.M + 127) / 128), dim3(256), lds, st, g);
    ASPIRE_LAUNCH_OK();
    return ASPIRE_OK;
}
// N = 768 GEMM + residual + LayerNorm in one launch (gemm_p_kernel's LN form): 128-wide column tiles, or 64-wide ones where the launch
// would otherwise leave workgroup slots empty (as launch_gemm_p chooses).  g.ln_count: this use's zeroed counters.
template <int BN>
int launch_gemm_p_ln_bn(PGemmArgs g, hipStream_t st) {
    constexpr int NS = 3, lds = NS * (kPTile + BN * kPRowBytes);
    static hipError_t raised = hipFuncSetAttribute(reinterpret_cast<const void*>(gemm_p_ln_kernel<BN>), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    ASPIRE_HIP_OK(raised);
    g.n_off = 0;
    g.probe = tuning().gemm_probe >= 32 ? tuning().gemm_probe - 32 : 0;      // 40 (timing experiment): nobody waits for its row block (wrong results); 48 (tests): a tile per row block never reports, its partners run into the wait's bound
    g.tiles_x = kD / BN;
    g.tiles_y = (g.M + 127) / 128;
    const unsigned per_xcd = (unsigned)((g.tiles_y + 7) / 8) * (unsigned)g.tiles_x;
    hipLaunchKernelGGL((gemm_p_ln_kernel<BN>), dim3(8 * per_xcd), dim3(256), lds, st, g);
    ASPIRE_LAUNCH_OK();
    return ASPIRE_OK;
}
int launch_gemm_p_ln(const PGemmArgs& g, hipStream_t st) {
    ASPIRE_REQUIRE(g.N == kD && g.K % 32 == 0 && g.resp && (g.C || g.Cp) && g.gamma && g.beta && g.ln_stats && g.ln_count, ASPIRE_ERR_INVALID_ARG,
                   "LayerNorm-epilogue GEMM: N = 768, a residual in the P layout, gamma / beta and the exchange buffers");
    // 128-wide column tiles whatever the row count: the 64-wide form (twelve tiles per row block to wait for, half the columns per wave)
    // measured 76 us against 36 + 14 for the plain 64-wide GEMM + layernorm_kernel at 8192 x 768 x 768; ASPIRE_HIP_GEMM_TILE=64 pins it (tests)
    if (tuning().gemm_tile == 64) return launch_gemm_p_ln_bn<64>(g, st);
    return launch_gemm_p_ln_bn<128>(g, st);
}
// The LayerNorm-epilogue form's forward-progress argument (gemm_p_ln_kernel) was made and measured on ONE part: gfx950 in SPX mode -- 256 CUs
// in 8 XCDs, workgroup id mod 8 = the XCD, three workgroups of this kernel per CU.  Anywhere else (another partition mode, CU masking that
// changes the CU count the runtime reports, another chip) the default is the separate layernorm_kernel pass; ASPIRE_HIP_GEMM_LN=on still pins
// the fused form (its wait is bounded either way).
bool ln_fused_supported() {
    static int cached[64];          // per device ordinal: 0 unknown, 1 yes, 2 no
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return false;
    if (!cached[dev]) {
        hipDeviceProp_t prop;
        bool ok = hipGetDeviceProperties(&prop, dev) == hipSuccess && !strncmp(prop.gcnArchName, "gfx950", 6) && prop.multiProcessorCount == 256;
        cached[dev] = ok ? 1 : 2;
    }
    return cached[dev] == 1;
}
// where a layer's four weight matrices sit in the prepared planes buffer
struct PlaneOffsets {
    size_t qkv, o, ffn1, ffn2, per_layer;
};
PlaneOffsets plane_offsets(int ffn_dim) {
    PlaneOffsets o{};
    size_t off = 0;
    o.qkv = off; off += align_up(p_bytes(3 * kD, kD));
    o.o = off; off += align_up(p_bytes(kD, kD));
    o.ffn1 = off; off += align_up(p_bytes(ffn_dim, kD));
    o.ffn2 = off; off += align_up(p_bytes(kD, ffn_dim));
    o.per_layer = off;
    return o;
}


// ---------------------------------------------------------------------------------------------------------------
// One forward's plan -- the form every step takes, decided once from B, L, the weights and the tuning pins -- and one layer of it.
// aspire_bert_forward_f32 runs every layer through run_layer; aspire_bert_forward_cls_f32 runs all but the last one the same way.
// ---------------------------------------------------------------------------------------------------------------
struct Fwd {
    const aspire_bert_weights* w;
    const int64_t* mask;
    int64_t B, L, M, row_tiles;
    int Lp, H, dh;
    unsigned row_blocks;
    bool pp, ln_fused, attn_p;
    PlaneOffsets po;
    Workspace ws;
    hipStream_t st;
};

// the forwards' argument checks: all of them before the first launch
int check_forward_args(const aspire_bert_weights* w, const int64_t* tok_ids, const int64_t* attn_mask, const float* out, int64_t B, int64_t L) {
    ASPIRE_REQUIRE(w && tok_ids && attn_mask && out, ASPIRE_ERR_INVALID_ARG, "null pointer");
    ASPIRE_REQUIRE(w->hidden == kD && w->n_heads == 12 && w->ffn_dim % 64 == 0 && w->ffn_dim > 0, ASPIRE_ERR_UNSUPPORTED,
                   "only BERT-base geometry is built (hidden 768, 12 heads); got hidden %d heads %d", w->hidden, w->n_heads);
    ASPIRE_REQUIRE(B >= 0 && L > 0 && L <= 512 && L <= w->max_pos, ASPIRE_ERR_INVALID_ARG,
                   "sequence length %lld outside (0, min(512, max_position_embeddings=%d)]", (long long)L, w->max_pos);
    ASPIRE_REQUIRE(w->n_layers >= 0 && (w->n_layers == 0 || w->layers), ASPIRE_ERR_INVALID_ARG, "bad layer table");
    return ASPIRE_OK;
}

int plan_forward(Fwd& f, const aspire_bert_weights* w, const int64_t* attn_mask, int64_t B, int64_t L, void* workspace, hipStream_t st) {
    f.w = w;
    f.mask = attn_mask;
    f.B = B;
    f.L = L;
    f.st = st;
    f.ws = carve(workspace, B, L, w->n_heads, w->ffn_dim, w->n_layers);
    f.M = B * L;
    f.Lp = (int)((L + 3) / 4 * 4);
    f.H = w->n_heads;
    f.dh = kD / f.H;
    f.row_blocks = (unsigned)((f.M + 3) / 4);
    // P path: the weights' planes are prepared (aspire_bert_prepare_planes), BERT-base shapes tile by 128 -- every nn.Linear GEMM
    // streams pre-split fp16 operands (gemm_p_kernel), from 1024 token rows on (measured B x L = 4 x 128: 2.46 vs 2.42 ms per batch,
    // 8 x 128: 2.55 vs 2.81, 16 x 128: 2.90 vs 3.52, 32 x 256: 6.64 vs 9.8); below -- and with ASPIRE_HIP_GEMM=f32 | bf16x3, or without
    // planes -- the round-2 kernels, which pick smaller tiles for small M
    f.pp = w->planes != nullptr && (tuning().gemm_form == 0 ? f.M >= 1024 : tuning().gemm_form == 3) && f.dh == 64 && !tuning().attn_gemm &&
           w->ffn_dim % 128 == 0;
    f.po = plane_offsets(w->ffn_dim);
    // LayerNorm in the N = 768 GEMMs' epilogue (ASPIRE_HIP_GEMM_LN=off: the separate layernorm_kernel pass)
    // from 48 row tiles on (measured, fused / separate ms per batch: 64 x 256 9.00 - 9.18 / 9.45, 128 x 128 8.99 / 9.40, 64 x 128 5.05 / 5.15,
    // 32 x 256 5.16 / 5.30, 40 x 100 3.09 / 3.17, 16 x 256 3.18 / 3.14, 8 x 256 2.37 / 2.30: below, the launch is a fraction of one round of
    // workgroups and a waiting workgroup has nothing running under it)
    f.row_tiles = (f.M + 127) / 128;
    f.ln_fused = f.pp && (tuning().gemm_ln == 2 || (tuning().gemm_ln == 0 && f.row_tiles >= 48 && ln_fused_supported()));
    // Round 6 (default on the plane path; ASPIRE_HIP_ATTN=f16x2 pins round 5's form, which splits fp32 Q / K / V inside the attention kernel):
    // the QKV GEMM writes the attention's operands as fp16 planes, the attention stages them by LDS-DMA (flash_attn_p_kernel)
    f.attn_p = f.pp && w->n_layers > 0 && tuning().attn_form != 1 && !tuning().attn_f32 && tuning().gemm_tile == 0;
    return ASPIRE_OK;
}

// embeddings + LayerNorm -> x (fp32) and, on the P path, actp; then the LayerNorm-epilogue counters of this forward
int launch_embed(const Fwd& f, const int64_t* tok_ids, const int64_t* type_ids, float* x) {
    const aspire_bert_weights* w = f.w;
    hipLaunchKernelGGL(embed_layernorm_kernel, dim3(f.row_blocks), dim3(256), 0, f.st, tok_ids, type_ids, w->word_emb, w->pos_emb,
                       w->type_emb, w->emb_ln_g, w->emb_ln_b, w->ln_eps, x, f.M, f.L, f.pp && w->n_layers > 0 ? f.ws.actp : nullptr);
    ASPIRE_LAUNCH_OK();
    // the P layout's slot offsets are 32-bit byte offsets (p_slot / p_slot8: ((k >> 4) R + r) << 6): the widest operand is [M, ffn_dim]
    ASPIRE_REQUIRE(!f.pp || (uint64_t)f.M * (uint64_t)(w->ffn_dim > 3 * kD ? w->ffn_dim : 3 * kD) * 4 < (1ull << 32), ASPIRE_ERR_UNSUPPORTED,
                   "%lld token rows in one forward: the fp16-plane layout addresses < 4 GB per operand (split the batch)", (long long)f.M);
    if (f.ln_fused && w->n_layers > 0) ASPIRE_HIP_OK(hipMemsetAsync(f.ws.ln_count, 0, f.ws.ln_count_bytes, f.st));
    return ASPIRE_OK;
}

// layer l: x (its input, fp32; on the fused form the input lives in actp) -> out.  last: out is the caller's [M, 768] and no P copy of
// it is written.  qkv_only: step 1 alone (the CLS forward's last layer)
int run_layer(const Fwd& f, int l, const float* x, float* out, bool last, bool qkv_only) {
    const aspire_bert_weights* w = f.w;
    const Workspace& ws = f.ws;
    const PlaneOffsets& po = f.po;
    const bool pp = f.pp, ln_fused = f.ln_fused, attn_p = f.attn_p;
    const int64_t B = f.B, L = f.L, M = f.M, row_tiles = f.row_tiles;
    const int Lp = f.Lp, H = f.H, dh = f.dh;
    const unsigned row_blocks = f.row_blocks;
    const int64_t* attn_mask = f.mask;
    hipStream_t st = f.st;
    const aspire_bert_layer& ly = w->layers[l];
    const char* lp = (const char*)w->planes + (size_t)l * po.per_layer;
    GemmArgs g{};
    PGemmArgs pg{};
    // 1. fused QKV projection: qkv [M, 2304] = x . Wqkv^T + bqkv
    if (attn_p) {
        // Q, K and V go out as the attention kernel's fp16 planes (no fp32 qkv exists in this form)
        pg = PGemmArgs{ws.actp, lp + po.qkv, nullptr, nullptr, ly.b_qkv, nullptr, (int)M, 3 * kD, kD, 0, 0, 0};
        pg.Xp = ws.qkvp;
        if (int rc = launch_gemm_p_qkv(pg, st)) return rc;
    } else if (pp) {
        pg = PGemmArgs{ws.actp, lp + po.qkv, ws.qkv, nullptr, ly.b_qkv, nullptr, (int)M, 3 * kD, kD, 3 * kD, 0, 0};
        if (int rc = launch_gemm_p<false>(pg, st)) return rc;
    } else {
        g = GemmArgs{};
        g.A = x; g.B = ly.w_qkv; g.C = ws.qkv; g.bias = ly.b_qkv;
        g.M = (int)M; g.N = 3 * kD; g.K = kD; g.lda = kD; g.ldb = kD; g.ldc = 3 * kD; g.nz2 = 1; g.alpha = 1.f;
        if (int rc = launch_gemm<false>(g, 1, st)) return rc;
    }
    if (qkv_only) return ASPIRE_OK;
    // 2-4. attention.  Fused kernel (scores never leave the chip) unless ASPIRE_HIP_ATTN=gemm pins the
    // three-kernel form (QK^T GEMM, masked soft-max, PV GEMM) that the fused one is tested against.
    if (attn_p) {
        const unsigned qblocks = (unsigned)((L + 127) / 128);
        if (tuning().attn_form == 2)
            hipLaunchKernelGGL(flash_attn_p64_kernel, dim3((unsigned)(B * H) * qblocks), dim3(256), 0, st, ws.qkvp, attn_mask, ws.ctx, (int)L, H, ws.ctxp, M);
        else
            hipLaunchKernelGGL(flash_attn_p_kernel, dim3((unsigned)(B * H) * qblocks), dim3(256), 0, st, ws.qkvp, attn_mask, ws.ctx, (int)L, H, ws.ctxp, M);
        ASPIRE_LAUNCH_OK();
    } else if (dh == 64 && !tuning().attn_gemm) {
        const unsigned qblocks = (unsigned)((L + 127) / 128);
        if (tuning().attn_f32)
            hipLaunchKernelGGL(flash_attn_f32_kernel, dim3((unsigned)(B * H) * qblocks), dim3(256), 0, st, ws.qkv, attn_mask, ws.ctx,
                               (int)L, H, pp ? ws.ctxp : nullptr, M);
        else
            hipLaunchKernelGGL(flash_attn_f16x2_kernel, dim3((unsigned)(B * H) * qblocks), dim3(256), 0, st, ws.qkv, attn_mask, ws.ctx,
                               (int)L, H, pp ? ws.ctxp : nullptr, M);
        ASPIRE_LAUNCH_OK();
    } else {
        // 2. scores[b,h] = Q_bh . K_bh^T   (scale and mask are applied by the softmax kernel)
        g = GemmArgs{};
        g.A = ws.qkv; g.B = ws.qkv + kD; g.C = ws.scores;
        g.M = (int)L; g.N = (int)L; g.K = dh; g.lda = 3 * kD; g.ldb = 3 * kD; g.ldc = Lp; g.nz2 = H; g.alpha = 1.f;
        g.sa1 = (long long)L * 3 * kD; g.sa2 = dh; g.sb1 = g.sa1; g.sb2 = dh;
        g.sc1 = (long long)H * L * Lp; g.sc2 = (long long)L * Lp;
        if (int rc = launch_gemm<false>(g, (int)(B * H), st)) return rc;
        // 3. masked softmax over keys
        const int64_t srows = B * H * L;
        hipLaunchKernelGGL(softmax_mask_kernel, dim3((unsigned)((srows + 3) / 4)), dim3(256), 0, st, ws.scores, attn_mask, srows,
                           (int)L, Lp, (int)(H * L), 1.0f / sqrtf((float)dh));
        ASPIRE_LAUNCH_OK();
        // 4. ctx[b, :, h*64:(h+1)*64] = P_bh . V_bh        (V is [K = L keys, N = 64] n-contiguous)
        g = GemmArgs{};
        g.A = ws.scores; g.B = ws.qkv + 2 * kD; g.C = ws.ctx;
        g.M = (int)L; g.N = dh; g.K = (int)L; g.lda = Lp; g.ldb = 3 * kD; g.ldc = kD; g.nz2 = H; g.alpha = 1.f;
        g.sa1 = (long long)H * L * Lp; g.sa2 = (long long)L * Lp; g.sb1 = (long long)L * 3 * kD; g.sb2 = dh;
        g.sc1 = (long long)L * kD; g.sc2 = dh;
        if (int rc = launch_gemm<true>(g, (int)(B * H), st)) return rc;
    }
    // 5. attention output projection + residual, LayerNorm
    if (ln_fused) {
        // x lives in actp (written by the embedding LayerNorm / the previous layer's FFN2 epilogue, read by the QKV GEMM): read as the
        // residual and replaced by h = LN1(.) slot by slot; no fp32 copy of x or h exists in this form
        pg = PGemmArgs{ws.ctxp, lp + po.o, nullptr, ws.actp, ly.b_o, nullptr, (int)M, kD, kD, kD, kD, 0};
        pg.resp = ws.actp;
        pg.gamma = ly.ln1_g; pg.beta = ly.ln1_b; pg.eps = w->ln_eps;
        pg.ln_stats = ws.ln_stats; pg.ln_count = ws.ln_count + (size_t)(2 * l) * row_tiles;
        if (int rc = launch_gemm_p_ln(pg, st)) return rc;
    } else if (pp) {
        pg = PGemmArgs{ws.ctxp, lp + po.o, ws.tmp, nullptr, ly.b_o, x, (int)M, kD, kD, kD, kD, 0};
        if (int rc = launch_gemm_p<false>(pg, st)) return rc;
    } else {
        g = GemmArgs{};
        g.A = ws.ctx; g.B = ly.w_o; g.C = ws.tmp; g.bias = ly.b_o; g.res = x; g.ldr = kD;
        g.M = (int)M; g.N = kD; g.K = kD; g.lda = kD; g.ldb = kD; g.ldc = kD; g.nz2 = 1; g.alpha = 1.f;
        if (int rc = launch_gemm<false>(g, 1, st)) return rc;
    }
    if (!ln_fused) {
        hipLaunchKernelGGL(layernorm_kernel, dim3(row_blocks), dim3(256), 0, st, ws.tmp, ly.ln1_g, ly.ln1_b, w->ln_eps, ws.ctx, M,
                           pp ? ws.actp : nullptr);
        ASPIRE_LAUNCH_OK();
    }
    // 6. FFN: GELU(h . W1^T + b1) . W2^T + b2 + h, LayerNorm          (h = ws.ctx)
    if (pp) {
        pg = PGemmArgs{ws.actp, lp + po.ffn1, nullptr, ws.ffnp, ly.b_ffn1, nullptr, (int)M, w->ffn_dim, kD, 0, 0, 0};
        if (int rc = launch_gemm_p<true>(pg, st)) return rc;
        if (ln_fused) {
            pg = PGemmArgs{ws.ffnp, lp + po.ffn2, last ? out : nullptr, last ? nullptr : ws.actp, ly.b_ffn2, nullptr, (int)M, kD, w->ffn_dim, kD, kD, 0};
            pg.resp = ws.actp;
            pg.gamma = ly.ln2_g; pg.beta = ly.ln2_b; pg.eps = w->ln_eps;
            pg.ln_stats = ws.ln_stats; pg.ln_count = ws.ln_count + (size_t)(2 * l + 1) * row_tiles;
            if (int rc = launch_gemm_p_ln(pg, st)) return rc;
        } else {
            pg = PGemmArgs{ws.ffnp, lp + po.ffn2, ws.tmp, nullptr, ly.b_ffn2, ws.ctx, (int)M, kD, w->ffn_dim, kD, kD, 0};
            if (int rc = launch_gemm_p<false>(pg, st)) return rc;
        }
    } else {
        g = GemmArgs{};
        g.A = ws.ctx; g.B = ly.w_ffn1; g.C = ws.ffn; g.bias = ly.b_ffn1; g.gelu = 1;
        g.M = (int)M; g.N = w->ffn_dim; g.K = kD; g.lda = kD; g.ldb = kD; g.ldc = w->ffn_dim; g.nz2 = 1; g.alpha = 1.f;
        if (int rc = launch_gemm<false>(g, 1, st)) return rc;
        g = GemmArgs{};
        g.A = ws.ffn; g.B = ly.w_ffn2; g.C = ws.tmp; g.bias = ly.b_ffn2; g.res = ws.ctx; g.ldr = kD;
        g.M = (int)M; g.N = kD; g.K = w->ffn_dim; g.lda = w->ffn_dim; g.ldb = w->ffn_dim; g.ldc = kD; g.nz2 = 1; g.alpha = 1.f;
        if (int rc = launch_gemm<false>(g, 1, st)) return rc;
    }
    if (!ln_fused) {
        hipLaunchKernelGGL(layernorm_kernel, dim3(row_blocks), dim3(256), 0, st, ws.tmp, ly.ln2_g, ly.ln2_b, w->ln_eps, out, M,
                           pp && !last ? ws.actp : nullptr);
        ASPIRE_LAUNCH_OK();
    }
    return ASPIRE_OK;
}

// The CLS forward's own workspace, behind the forward's (carve): the B gathered rows of the last layer
struct ClsWorkspace {
    float *gin, *ctx, *tmp, *h, *y, *ffn;      // residual input (hidden state n - 1), attention context, pre-norm, LN1, LN2, GELU(FFN1)
    size_t total;
};
ClsWorkspace carve_cls(void* base, int64_t B, int ffn_dim) {
    char* p = (char*)base;
    ClsWorkspace c;
    size_t off = 0;
    auto take = [&](size_t nfloats) {
        float* r = (float*)(p + off);
        off += align_up(nfloats * sizeof(float));
        return r;
    };
    c.gin = take((size_t)B * kD);
    c.ctx = take((size_t)B * kD);
    c.tmp = take((size_t)B * kD);
    c.h = take((size_t)B * kD);
    c.y = take((size_t)B * kD);
    c.ffn = take((size_t)B * ffn_dim);
    c.total = off;
    return c;
}

// The CLS row (row b L) of each of the B documents of one hidden state, read from fp32 x [rows, 768] or from the P-layout planes xp
// (the fused-LayerNorm form's actp: p_slot, as the GEMMs that write it): -> layer_cls [B, 768] and gather [B, 768] (each optional);
// mode 1: cls_out = wt x row, 2: cls_out += wt x row, 0: cls_out untouched.  One wave per document.
__global__ void __launch_bounds__(256) cls_tap_kernel(const float* __restrict__ x, const void* __restrict__ xp, int64_t rows, int64_t L,
                                                      int64_t B, float wt, int mode, float* __restrict__ cls_out,
                                                      float* __restrict__ layer_cls, float* __restrict__ gather) {
    const int lane = threadIdx.x & 63;
    const int64_t b = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= B) return;
    const int64_t r = b * L;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const int d = 4 * lane + 256 * c;
        const float4 v = xp ? p_load4_at(xp, p_slot((uint32_t)rows, (uint32_t)r, (uint32_t)d)) : *reinterpret_cast<const float4*>(x + r * kD + d);
        const size_t o = (size_t)b * kD + d;
        if (layer_cls) *reinterpret_cast<float4*>(layer_cls + o) = v;
        if (gather) *reinterpret_cast<float4*>(gather + o) = v;
        if (mode) {
            float4 a = make_float4(wt * v.x, wt * v.y, wt * v.z, wt * v.w);
            if (mode == 2) {
                const float4 p = *reinterpret_cast<const float4*>(cls_out + o);
                a = make_float4(p.x + a.x, p.y + a.y, p.z + a.z, p.w + a.w);
            }
            *reinterpret_cast<float4*>(cls_out + o) = a;
        }
    }
}

// Attention of the CLS query alone, one workgroup per (document, head): softmax_j(q . k_j / 8 + (mask_j ? 0 : finfo.min)) v_j over the
// document's L <= 512 keys, in fp32 (the scores and the mask bias as softmax_mask_kernel forms them).  Q / K / V come from the fp32 qkv
// [rows, 2304] of the round-2 / f32 / f16x2 forms, or (qkvp != NULL) from the planes [plane h | l][Q | K | V][head][rows][64] fp16 that
// launch_gemm_p_qkv writes for flash_attn_p_kernel.  ctx [B, 768]: head h at columns 64 h .. + 63.
__device__ __forceinline__ void cls_attn_row(const float* qkv, const unsigned char* qkvp, int which, int H, int h, int64_t rows, int64_t row,
                                             float (&v)[64]) {
    if (qkvp) {
        const size_t plane_b = (size_t)3 * H * rows * 128;
        const unsigned char* p = qkvp + ((size_t)(which * H + h) * rows + row) * 128;
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            const f16x8_t hi = *reinterpret_cast<const f16x8_t*>(p + 16 * c), lo = *reinterpret_cast<const f16x8_t*>(p + plane_b + 16 * c);
#pragma unroll
            for (int e = 0; e < 8; ++e) v[8 * c + e] = (float)hi[e] + (float)lo[e];
        }
    } else {
        const float* p = qkv + row * 3 * kD + which * kD + h * 64;
#pragma unroll
        for (int c = 0; c < 16; ++c) {
            const float4 t = *reinterpret_cast<const float4*>(p + 4 * c);
            v[4 * c] = t.x, v[4 * c + 1] = t.y, v[4 * c + 2] = t.z, v[4 * c + 3] = t.w;
        }
    }
}
__device__ __forceinline__ float cls_attn_elem(const float* qkv, const unsigned char* qkvp, int which, int H, int h, int64_t rows, int64_t row, int d) {
    if (qkvp) {
        const unsigned char* p = qkvp + ((size_t)(which * H + h) * rows + row) * 128 + 2 * d;
        return (float)*reinterpret_cast<const _Float16*>(p) + (float)*reinterpret_cast<const _Float16*>(p + (size_t)3 * H * rows * 128);
    }
    return qkv[row * 3 * kD + which * kD + h * 64 + d];
}
__global__ void __launch_bounds__(256) cls_attn_kernel(const float* __restrict__ qkv, const unsigned char* __restrict__ qkvp,
                                                       const int64_t* __restrict__ mask, float* __restrict__ ctx, int L, int H, int64_t rows) {
    __shared__ float qs[64];
    __shared__ float pr[512];
    __shared__ float red[4];
    __shared__ float part[4][64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int h = (int)(blockIdx.x % H);
    const int64_t b = blockIdx.x / H, doc0 = b * L;
    if (tid < 64) qs[tid] = cls_attn_elem(qkv, qkvp, 0, H, h, rows, doc0, tid);
    __syncthreads();
    // scores: thread t takes keys t and t + 256
    float m = -INFINITY;
    for (int j = tid; j < L; j += 256) {
        float k[64];
        cls_attn_row(qkv, qkvp, 1, H, h, rows, doc0 + j, k);
        float s = 0.f;
#pragma unroll
        for (int d = 0; d < 64; ++d) s = fmaf(qs[d], k[d], s);
        s = s * 0.125f + (mask[doc0 + j] != 0 ? 0.f : -3.4028234663852886e38f);
        pr[j] = s;
        m = fmaxf(m, s);
    }
    m = wave_max(m);
    if (lane == 0) red[wave] = m;
    __syncthreads();
    m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    __syncthreads();
    float sum = 0.f;
    for (int j = tid; j < L; j += 256) {
        const float e = expf(pr[j] - m);
        pr[j] = e;
        sum += e;
    }
    sum = wave_sum(sum);
    if (lane == 0) red[wave] = sum;
    __syncthreads();
    const float inv = 1.0f / ((red[0] + red[1]) + (red[2] + red[3]));
    // context: wave w sums keys w, w + 4, ..; lane = dim
    float acc = 0.f;
    for (int j = wave; j < L; j += 4) acc = fmaf(pr[j], cls_attn_elem(qkv, qkvp, 2, H, h, rows, doc0 + j, lane), acc);
    part[wave][lane] = acc;
    __syncthreads();
    if (tid < 64) ctx[b * kD + h * 64 + tid] = ((part[0][tid] + part[1][tid]) + (part[2][tid] + part[3][tid])) * inv;
}

}  // namespace
}  // namespace aspire

using namespace aspire;

extern "C" size_t aspire_bert_workspace_bytes(const aspire_bert_weights* w, int64_t B, int64_t L) {
    if (!w || B <= 0 || L <= 0) return 0;
    return carve(nullptr, B, L, w->n_heads, w->ffn_dim, w->n_layers).total;
}

extern "C" int aspire_bert_forward_f32(const aspire_bert_weights* w, const int64_t* tok_ids, const int64_t* type_ids,
                                       const int64_t* attn_mask, int64_t B, int64_t L, float* hidden_out, void* workspace,
                                       size_t workspace_bytes, void* stream) {
    if (int rc = check_forward_args(w, tok_ids, attn_mask, hidden_out, B, L)) return rc;
    if (B == 0) return ASPIRE_OK;
    const size_t need = carve(nullptr, B, L, w->n_heads, w->ffn_dim, w->n_layers).total;
    ASPIRE_REQUIRE(workspace && workspace_bytes >= need, ASPIRE_ERR_INVALID_ARG, "workspace too small: need %zu bytes", need);
    Fwd f;
    if (int rc = plan_forward(f, w, attn_mask, B, L, workspace, (hipStream_t)stream)) return rc;
    float* x = w->n_layers == 0 ? hidden_out : f.ws.x;
    if (int rc = launch_embed(f, tok_ids, type_ids, x)) return rc;
    for (int l = 0; l < w->n_layers; ++l) {
        const bool last = l == w->n_layers - 1;
        float* out = last ? hidden_out : f.ws.x;  // LN2 writes the layer output (x is dead by then)
        if (int rc = run_layer(f, l, x, out, last, false)) return rc;
        x = out;
    }
    return ASPIRE_OK;
}

extern "C" size_t aspire_bert_cls_workspace_bytes(const aspire_bert_weights* w, int64_t B, int64_t L) {
    if (!w || B <= 0 || L <= 0) return 0;
    const size_t base = carve(nullptr, B, L, w->n_heads, w->ffn_dim, w->n_layers).total;
    return base + carve_cls(nullptr, B, w->ffn_dim).total;
}

// The CLS rows of every hidden state and their mix (ex_aspire_bienc.py:23-58, disent_models.py:183-205): layers 0 .. n - 2 are
// aspire_bert_forward_f32's own launches; after the embedding LayerNorm and after every layer cls_tap_kernel reads the B CLS rows
// where that form left them (fp32 x, or the fp16 planes of actp on the fused-LayerNorm form) and adds w_l x row to cls_out.  The last
// layer runs its QKV GEMM over all rows, then ONE query per (document, head) (cls_attn_kernel) and the rest of the layer on the B
// gathered rows only: nothing after the keys and values of a non-CLS row is ever read.
extern "C" int aspire_bert_forward_cls_f32(const aspire_bert_weights* w, const int64_t* tok_ids, const int64_t* type_ids,
                                           const int64_t* attn_mask, int64_t B, int64_t L, const float* layer_mix, float* cls_out,
                                           float* layer_cls, void* workspace, size_t workspace_bytes, void* stream) {
    if (int rc = check_forward_args(w, tok_ids, attn_mask, cls_out, B, L)) return rc;
    if (layer_mix)
        for (int i = 0; i <= w->n_layers; ++i)
            ASPIRE_REQUIRE(isfinite(layer_mix[i]), ASPIRE_ERR_INVALID_ARG, "layer_mix[%d] is not finite", i);
    if (B == 0) return ASPIRE_OK;
    const size_t need = aspire_bert_cls_workspace_bytes(w, B, L);
    ASPIRE_REQUIRE(workspace && workspace_bytes >= need, ASPIRE_ERR_INVALID_ARG, "workspace too small: need %zu bytes", need);
    Fwd f;
    if (int rc = plan_forward(f, w, attn_mask, B, L, workspace, (hipStream_t)stream)) return rc;
    const ClsWorkspace cw = carve_cls((char*)workspace + f.ws.total, B, w->ffn_dim);
    const int n = w->n_layers;
    const unsigned tap_blocks = (unsigned)((B + 3) / 4);
    // hidden state i: its CLS row -> layer_cls[i], cls_out (+)= mix[i] x row, and (i = n - 1) the last layer's residual input
    auto tap = [&](int i, const float* x, const void* xp, int64_t rows, int64_t ld_rows) -> int {
        const int mode = layer_mix ? (i == 0 ? 1 : 2) : (i == n ? 1 : 0);
        const float wt = layer_mix ? layer_mix[i] : 1.f;
        hipLaunchKernelGGL(cls_tap_kernel, dim3(tap_blocks), dim3(256), 0, f.st, x, xp, rows, ld_rows, B, wt, mode, cls_out,
                           layer_cls ? layer_cls + (size_t)i * B * kD : nullptr, i == n - 1 ? cw.gin : nullptr);
        ASPIRE_LAUNCH_OK();
        return ASPIRE_OK;
    };
    if (int rc = launch_embed(f, tok_ids, type_ids, f.ws.x)) return rc;
    if (int rc = tap(0, f.ws.x, nullptr, f.M, L)) return rc;
    for (int l = 0; l + 1 < n; ++l) {
        if (int rc = run_layer(f, l, f.ws.x, f.ws.x, false, false)) return rc;
        // the fused form keeps a layer's output only as the planes of actp; the others write fp32 x
        if (int rc = f.ln_fused ? tap(l + 1, nullptr, f.ws.actp, f.M, L) : tap(l + 1, f.ws.x, nullptr, f.M, L)) return rc;
    }
    if (n == 0) return ASPIRE_OK;
    // the last layer: Q, K, V of every row as the forward's attention form lays them out ...
    const aspire_bert_layer& ly = w->layers[n - 1];
    if (int rc = run_layer(f, n - 1, f.ws.x, f.ws.x, true, true)) return rc;
    hipLaunchKernelGGL(cls_attn_kernel, dim3((unsigned)(B * f.H)), dim3(256), 0, f.st, f.attn_p ? nullptr : f.ws.qkv,
                       f.attn_p ? f.ws.qkvp : nullptr, attn_mask, cw.ctx, (int)L, f.H, f.M);
    ASPIRE_LAUNCH_OK();
    // ... then the rest of the layer on the B context rows: out-proj + residual, LN1, GELU(FFN1), FFN2 + residual, LN2
    GemmArgs g{};
    g.A = cw.ctx; g.B = ly.w_o; g.C = cw.tmp; g.bias = ly.b_o; g.res = cw.gin; g.ldr = kD;
    g.M = (int)B; g.N = kD; g.K = kD; g.lda = kD; g.ldb = kD; g.ldc = kD; g.nz2 = 1; g.alpha = 1.f;
    if (int rc = launch_gemm<false>(g, 1, f.st)) return rc;
    hipLaunchKernelGGL(layernorm_kernel, dim3(tap_blocks), dim3(256), 0, f.st, cw.tmp, ly.ln1_g, ly.ln1_b, w->ln_eps, cw.h, B, nullptr);
    ASPIRE_LAUNCH_OK();
    g = GemmArgs{};
    g.A = cw.h; g.B = ly.w_ffn1; g.C = cw.ffn; g.bias = ly.b_ffn1; g.gelu = 1;
    g.M = (int)B; g.N = w->ffn_dim; g.K = kD; g.lda = kD; g.ldb = kD; g.ldc = w->ffn_dim; g.nz2 = 1; g.alpha = 1.f;
    if (int rc = launch_gemm<false>(g, 1, f.st)) return rc;
    g = GemmArgs{};
    g.A = cw.ffn; g.B = ly.w_ffn2; g.C = cw.tmp; g.bias = ly.b_ffn2; g.res = cw.h; g.ldr = kD;
    g.M = (int)B; g.N = kD; g.K = w->ffn_dim; g.lda = w->ffn_dim; g.ldb = w->ffn_dim; g.ldc = kD; g.nz2 = 1; g.alpha = 1.f;
    if (int rc = launch_gemm<false>(g, 1, f.st)) return rc;
    hipLaunchKernelGGL(layernorm_kernel, dim3(tap_blocks), dim3(256), 0, f.st, cw.tmp, ly.ln2_g, ly.ln2_b, w->ln_eps, cw.y, B, nullptr);
    ASPIRE_LAUNCH_OK();
    return tap(n, cw.y, nullptr, B, 1);
}

extern "C" int aspire_bert_status(int32_t* status_host, void* stream) {
    ASPIRE_REQUIRE(status_host, ASPIRE_ERR_INVALID_ARG, "null pointer");
    hipStream_t st = (hipStream_t)stream;
    int v = 0;
    const int zero = 0;
    ASPIRE_HIP_OK(hipMemcpyFromSymbolAsync(&v, HIP_SYMBOL(g_bert_status), sizeof(int), 0, hipMemcpyDeviceToHost, st));
    ASPIRE_HIP_OK(hipStreamSynchronize(st));
    if (v) {
        ASPIRE_HIP_OK(hipMemcpyToSymbolAsync(HIP_SYMBOL(g_bert_status), &zero, sizeof(int), 0, hipMemcpyHostToDevice, st));
        ASPIRE_HIP_OK(hipStreamSynchronize(st));
    }
    *status_host = v;
    return ASPIRE_OK;
}

// The weights' fp16 planes, formed ONCE when the model is loaded: a device buffer of aspire_bert_planes_bytes(w) bytes that the
// caller keeps next to the weights and hands over as aspire_bert_weights::planes.
extern "C" size_t aspire_bert_planes_bytes(const aspire_bert_weights* w) {
    if (!w || w->n_layers <= 0 || w->hidden != kD || w->ffn_dim <= 0) return 0;
    return plane_offsets(w->ffn_dim).per_layer * (size_t)w->n_layers;
}

extern "C" int aspire_bert_prepare_planes(const aspire_bert_weights* w, void* planes, size_t planes_bytes, void* stream) {
    ASPIRE_REQUIRE(w && planes, ASPIRE_ERR_INVALID_ARG, "null pointer");
    ASPIRE_REQUIRE(w->hidden == kD && w->ffn_dim % 128 == 0 && w->ffn_dim > 0, ASPIRE_ERR_UNSUPPORTED,
                   "pre-split weights are built for hidden 768 and an ffn width that is a multiple of 128");
    ASPIRE_REQUIRE(planes_bytes >= aspire_bert_planes_bytes(w), ASPIRE_ERR_INVALID_ARG, "planes buffer too small");
    hipStream_t st = (hipStream_t)stream;
    const PlaneOffsets po = plane_offsets(w->ffn_dim);
    int* too_big = nullptr;        // a load-time call: its own 4 bytes, one synchronisation at the end
    ASPIRE_HIP_OK(hipMalloc((void**)&too_big, sizeof(int)));
    auto split = [&](const float* X, int64_t R, int K, void* P) {
        hipLaunchKernelGGL(split_planes_kernel, dim3((unsigned)((R * (K / 4) + 255) / 256)), dim3(256), 0, st, X, R, K, K, P, kPWeightScale,
                           too_big);
    };
    hipError_t e0 = hipMemsetAsync(too_big, 0, sizeof(int), st);
    if (e0 == hipSuccess) e0 = hipMemsetAsync(planes, 0, aspire_bert_planes_bytes(w), st);      // the slack rows behind every matrix
    if (e0 != hipSuccess) {
        (void)hipFree(too_big);
        ASPIRE_HIP_OK(e0);
    }
    for (int l = 0; l < w->n_layers; ++l) {
        const aspire_bert_layer& ly = w->layers[l];
        char* lp = (char*)planes + (size_t)l * po.per_layer;
        split(ly.w_qkv, 3 * kD, kD, lp + po.qkv);
        split(ly.w_o, kD, kD, lp + po.o);
        split(ly.w_ffn1, w->ffn_dim, kD, lp + po.ffn1);
        split(ly.w_ffn2, kD, w->ffn_dim, lp + po.ffn2);
    }
    int flag = 0;
    hipError_t e1 = hipGetLastError();
    if (e1 == hipSuccess) e1 = hipMemcpyAsync(&flag, too_big, sizeof(int), hipMemcpyDeviceToHost, st);
    if (e1 == hipSuccess) e1 = hipStreamSynchronize(st);
    (void)hipFree(too_big);
    ASPIRE_HIP_OK(e1);
    ASPIRE_REQUIRE(flag == 0, ASPIRE_ERR_UNSUPPORTED,
                   "a weight is not finite or beyond +-1023: outside the fp16-plane GEMM's range (leave aspire_bert_weights::planes NULL for such a model)");
    return ASPIRE_OK;
}

// Tuning hooks (not part of include/aspire_hip.h): an operand into the P layout (weight != 0: the B side, scaled), and one C = A . B^T (+bias) GEMM on P operands
// (tools/gemmbench.py); swap != 0: the GELU -> P-layout epilogue (Cp [M, N]).
extern "C" size_t aspire_debug_planes_bytes(int64_t R, int64_t K) { return p_bytes(R, K); }
extern "C" int aspire_debug_split_planes(const float* X, int64_t R, int K, void* P, int weight, void* stream) {
    ASPIRE_REQUIRE(K % 32 == 0, ASPIRE_ERR_UNSUPPORTED, "K %% 32");
    hipLaunchKernelGGL(split_planes_kernel, dim3((unsigned)((R * (K / 4) + 255) / 256)), dim3(256), 0, (hipStream_t)stream, X, R, K, K, P,
                       weight ? kPWeightScale : 1.0f, nullptr);
    ASPIRE_LAUNCH_OK();
    return ASPIRE_OK;
}
extern "C" int aspire_debug_gemm_planes(const void* Ap, const void* Bp, float* C, void* Cp, const float* bias, int M, int N, int K, int swap,
                                        void* stream) {
    PGemmArgs pg{Ap, Bp, C, Cp, bias, nullptr, M, N, K, N, 0, 0};
    return swap ? launch_gemm_p<true>(pg, (hipStream_t)stream) : launch_gemm_p<false>(pg, (hipStream_t)stream);
}

// Tuning hook (not part of include/aspire_hip.h): one plain C = A . B^T (+bias) GEMM through the encoder's tile
// dispatch, for tools/gemmbench.py.  A [M,K], B [N,K], C [M,N], all row-major fp32 device pointers.
extern "C" int aspire_debug_gemm_f32(const float* A, const float* B, float* C, const float* bias, int M, int N, int K,
                                     void* stream) {
    GemmArgs g{};
    g.A = A; g.B = B; g.C = C; g.bias = bias; g.res = nullptr;
    g.M = M; g.N = N; g.K = K;
    g.lda = K; g.ldb = K; g.ldc = N; g.ldr = 0;
    g.nz2 = 1;
    g.alpha = 1.0f;
    g.gelu = 0;
    return launch_gemm<false>(g, 1, (hipStream_t)stream);
}

#ifdef ASPIRE_PHASE_CLOCK
extern "C" void aspire_debug_gemm_buffer(void* p) {
    long long* q = (long long*)p;
    (void)hipMemcpyToSymbol(HIP_SYMBOL(aspire::g_gdbg), &q, sizeof(q));
}
#endif
