// The encoder's GEMMs on fp32 operands (round 2): what the forward takes below 1024 token rows or without prepared planes, the batched
// products of the three-kernel attention, the CLS forward's tail, and the A/B forms ASPIRE_HIP_GEMM=f32 | bf16x3.
//
// Kernels
//   gemm_f32_kernel          C = alpha * A.B^T (+bias)(+GELU)(+residual), batched/strided; A [M,K] k-contiguous,
//                            B either [N,K] k-contiguous (nn.Linear weight, K^T of attention) or [K,N]
//                            n-contiguous (V of attention).  128x128 / 128x96 / 128x64 / 64x64 block tiles, BK = 16,
//                            4 waves, LDS tiles stored k-major so MFMA operand reads are
//                            conflict-free ds_read_b32, register-staged double buffering.
//   gemm_bf16x3_kernel       the same for nn.Linear shapes on the bf16 matrix pipe: three bf16 planes per operand, split when a tile is
//                            staged, six products per term
//                            A_KM: the TN form, C[M, N] = sum_r A[r, M] . B[r, N] -- both operands row-major with the contraction over
//                            their rows (the encoder backward's dW = dY^T . X, dV = P^T . dO, dK = dS^T . Q); new instantiations of the
//                            same kernel, the existing ones keep their arithmetic.  The contraction is over token rows, so this
//                            form alone sums in two levels: the accumulators are folded into a second set every 256 rows
// Launch rules: launch_gemm (tile and form by shape and the ASPIRE_HIP_GEMM / ASPIRE_HIP_GEMM_TILE pins), launch_gemm_tn.
#include "enc_types.h"
#include "tuning.h"

namespace aspire {
namespace {

// A_KM (the TN form, launch_gemm_tn): A is [K, M] m-contiguous as well -- C[M, N] = sum_r A[r, M] . B[r, N], both operands row-major with
// the contraction over their rows (dW = dY^T . X, dV = P^T . dO, dK = dS^T . Q).  A row of either operand IS a row of its k-major LDS
// tile: float4 loads along m / n, float4 LDS stores, no transposing scatter -- B_KN's staging on both sides.
template <int BM, int BN, int kBK, bool B_KN, int WAVES_N = 2, bool A_KM = false>
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
            if constexpr (A_KM) {
                constexpr int M4 = BM / 4;
                const int idx = tid + 256 * p, kr = idx / M4, m4 = idx % M4;
                const int k = k0 + kr, m = m0 + 4 * m4;
                ra[p] = (k < g.K && m < g.M) ? *reinterpret_cast<const float4*>(A + (size_t)k * g.lda + m)
                                             : make_float4(0.f, 0.f, 0.f, 0.f);
            } else {
                const int idx = tid + 256 * p, row = idx / (kBK / 4), k4 = idx % (kBK / 4);
                const int m = m0 + row, k = k0 + 4 * k4;
                ra[p] = (m < g.M && k < g.K) ? *reinterpret_cast<const float4*>(A + (size_t)m * g.lda + k)
                                             : make_float4(0.f, 0.f, 0.f, 0.f);
            }
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
            if constexpr (A_KM) {
                constexpr int M4 = BM / 4;
                const int idx = tid + 256 * p, kr = idx / M4, m4 = idx % M4;
                *reinterpret_cast<float4*>(&As[buf][kr][4 * m4]) = ra[p];
            } else {
                const int idx = tid + 256 * p, row = idx / (kBK / 4), k4 = idx % (kBK / 4);
                As[buf][4 * k4 + 0][row] = ra[p].x;
                As[buf][4 * k4 + 1][row] = ra[p].y;
                As[buf][4 * k4 + 2][row] = ra[p].z;
                As[buf][4 * k4 + 3][row] = ra[p].w;
            }
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
    auto mma_tile = [&](int t) {
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
    };
    if constexpr (A_KM) {
        // The contraction runs over token rows -- thousands under training, where one fp32 accumulator summed in k order drifts by
        // the roundings of an ever larger running sum (a weight gradient over 5 599 rows was 6 - 9 x further from float64 than an
        // fp32 CPU GEMM).  So two levels: after every kFold k tiles (256 rows) the accumulators are added to `tot` and start again
        // from zero -- in a loop of its own around the tile loop, so that the tile loop stays what it was (a fold predicated inside
        // it is if-converted: every tile then drains the MFMAs to read the accumulators).  Up to 256 rows: the bits of one level.
        constexpr int kFold = 16;
        f32x16 tot[TM][TN];
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) tot[i][j][r] = 0.f;
        for (int t0 = 0; t0 < nk; t0 += kFold) {
            const int t1 = min(t0 + kFold, nk);
            for (int t = t0; t < t1; ++t) mma_tile(t);
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        tot[i][j][r] += acc[i][j][r];
                        acc[i][j][r] = 0.f;
                    }
        }
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j) acc[i][j] = tot[i][j];
    } else {
        for (int t = 0; t < nk; ++t) mma_tile(t);
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

// fraction of the last round of workgroups that runs empty, at 3 resident workgroups per CU
double gemm_rounds_waste(long long blocks) {
    const double rounds = (double)blocks / 768.0;
    const double full = (double)((blocks + 767) / 768);
    return (full - rounds) / full;
}

template <bool B_KN>
int launch_gemm_bkn(const GemmArgs& g, int batch, hipStream_t st) {
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

}  // namespace

int launch_gemm(const GemmArgs& g, int batch, bool b_kn, hipStream_t st) {
    return b_kn ? launch_gemm_bkn<true>(g, batch, st) : launch_gemm_bkn<false>(g, batch, st);
}

// The TN form (the encoder backward's weight gradients and dV / dK): A [K, M] and B [K, N], both row-major, M and N multiples of 4
// (float4 along m / n).  Tiles by the same rule as the fp32 forms above.
int launch_gemm_tn(const GemmArgs& g, int batch, hipStream_t st) {
    const long long b128 = (long long)((g.M + 127) / 128) * ((g.N + 127) / 128) * batch;
    const long long b12864 = (long long)((g.M + 127) / 128) * ((g.N + 63) / 64) * batch;
    if (b128 >= 512 && g.N >= 128) {
        hipLaunchKernelGGL((gemm_f32_kernel<128, 128, 16, true, 2, true>), dim3((g.N + 127) / 128, (g.M + 127) / 128, batch), dim3(256), 0, st, g);
    } else if (b12864 >= 512) {
        hipLaunchKernelGGL((gemm_f32_kernel<128, 64, 16, true, 2, true>), dim3((g.N + 63) / 64, (g.M + 127) / 128, batch), dim3(256), 0, st, g);
    } else {
        hipLaunchKernelGGL((gemm_f32_kernel<64, 64, 16, true, 2, true>), dim3((g.N + 63) / 64, (g.M + 63) / 64, batch), dim3(256), 0, st, g);
    }
    ASPIRE_LAUNCH_OK();
    return ASPIRE_OK;
}

}  // namespace aspire
