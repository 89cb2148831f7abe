// The training encoder's k-major matrix products at fp32 accuracy on the bf16 matrix pipe (the opt-in mode ASPIRE_MATMUL_BF16X3): one
// GEMM on v_mfma_f32_32x32x16_bf16 in the two operand forms that have a k-major operand, taking the GemmArgs of launch_gemm /
// launch_gemm_tn -- batched and strided, alpha, bias, GELU and residual epilogues in fp32, fp32 output.  It is gemm_bf16x3_kernel
// (enc_gemm.hip, the NT form, which only takes k-contiguous operands) for the other two forms:
//   B_KN  A [M, K] k-contiguous, B [K, N] n-contiguous     P V, every dX = dY W, dQ = dS K
//   TN    A [K, M], B [K, N], both k-major                  every dW = dY^T X, dV = P^T dctx, dK = dS^T Q
// The NT form of the mode is launch_gemm's: gemm_bf16x3_kernel whenever K % 16 == 0, which every NT product of the layer stack is.
//
// The arithmetic of the mode, and nothing else:
//   * every operand element is split ONCE, when its tile is staged from the fp32 tensor into LDS, into three bf16 planes
//     x = x1 + x2 + x3 (split3_bf16, common.h: x1 = bf16(x), x2 = bf16(x - x1), x3 = bf16(x - x1 - x2); 24 mantissa bits, both
//     subtractions exact);
//   * a product a b is the six terms a3 b1, a1 b3, a2 b2, a2 b1, a1 b2, a1 b1 in that order (smallest first), each exact in fp32; the
//     three dropped terms are below 2^-23 |a| |b| (|a2| <= 2^-8 |a|, |a3| <= 2^-16 |a|), of the order of fp32's own rounding;
//   * sums are the MFMA's fp32 accumulators in a fixed order: per 16 k, term by term, into TWO accumulators per output element -- `lo`
//     takes the five correction terms, `acc` takes a1 b1 -- and C = acc + lo, one fp32 add.  (With all six terms in one accumulator
//     the mode missed the fp32 mode's bound: the matrix core aligns an instruction's 16 products to its largest addend and cuts what
//     lies below its guard bits, toward minus infinity -- measured -0.002 ulp of the running sum per instruction.  Five of six
//     instructions add terms 2^-8 .. 2^-16 of the sum to it, all of them cut.  Nothing for one element, but the same sign in every
//     element: a column sum over token rows collects it, and the LayerNorm gain gradients of the trained-statistics case came out at
//     1.35 and 1.56 x their bound, where the fp32-input GEMMs sit at 0.35 and 0.24.  In `lo` the correction terms meet a sum of their own
//     size; `acc` takes one instruction per 16 k, fewer roundings than the fp32-input form's eight.  NOTES.md.)  The B_KN form sums
//     in ONE level, as gemm_f32_kernel's B_KN form does.  The TN form contracts over token rows and keeps gemm_f32_kernel's TWO
//     levels: every 256 k acc + lo is added to a second set and both start again from zero (one running fp32 sum over thousands of
//     rows drifts);
//   * the epilogue (alpha, bias, GELU, residual) is fp32, the other GEMMs';
//   * no atomics, one writer per output element: the same bits on every run.
// Any M, N, K: tails are zero-filled when a tile is staged (a partial float4 is read element by element, never past the operand's
// valid extent; a zero splits into three zero planes); lda / ldb multiples of 4 and 16-byte aligned bases, as the fp32 forms ask.
// Non-finite operands behave as in gemm_bf16x3_kernel: the split of an infinity has a NaN plane (inf - inf), so an infinite or NaN
// operand element makes its whole output row (or column) NaN.  A magnitude that rounds past bf16's largest finite does the same.
//
// Staging: StageRegs of enc_stage.h with three planes -- enc_gemm_bf16.hip's loads, register turn and row swizzle, split3_bf16 in
// the place of the one rounding.  16 k per tile (one MFMA step of every term): 48.8 KB of LDS at 128 x 128 double buffered, three
// workgroups per CU (gemm_bf16x3_kernel measured 16 k at three per CU ahead of 32 k at two).  A k-major 128-row tile of 16 k is 128
// blocks of 4 k x 4 rows: in the TN form the lower half of the workgroup stages A and the upper half B.
// Pipeline, gemm_bf16x3_kernel's: global loads run two tiles ahead, the split and the LDS stores of the next tile are threaded between
// this tile's MFMAs, one barrier per tile.  A load past K reads nothing and stages zeros, so the loop body has no tail case.
// Tiles 128 x 128, 128 x 64 and 64 x 64, four waves as 2 x 2.
#include <atomic>

#include "enc_host.h"
#include "enc_stage.h"
#include "tuning.h"

namespace aspire {
namespace {

constexpr int kX3BK = 16;        // k per tile: two groups of eight, one MFMA step
constexpr int kX3Fold = 16;      // TN: k tiles per fold of the accumulators (256 k, gemm_f32_kernel's)

// a 128 x 128 tile holds two accumulator sets of 64 registers, the TN form's a third: one wave per SIMD with all 512 registers, no spill
template <int BM, int BN, int FORM>
__global__ void __launch_bounds__(256, BM * BN == 128 * 128 ? 1 : 2) gemm_bf16x3_km_kernel(GemmArgs g) {
    static_assert(FORM == kGemmBKN || FORM == kGemmTN, "the forms with a k-major operand");
    constexpr bool A_KM = FORM == kGemmTN;
    constexpr int WAVES_N = 2;
    constexpr int WM = BM / 2, WN = BN / 2, TM = WM / 32, TN = WN / 32;
    static_assert(WM % 32 == 0 && WN % 32 == 0, "tile / wave layout");
    using StageA = StageRegs<BM, A_KM, kX3BK, 3>;
    using StageB = StageRegs<BN, true, kX3BK, 3>;
    __shared__ __attribute__((aligned(16))) uint32_t As[2][3][2][StageA::kPlane];
    __shared__ __attribute__((aligned(16))) uint32_t Bs[2][3][2][StageB::kPlane];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wr = wave / WAVES_N, wc = wave % WAVES_N;
    const int tid_b = A_KM ? tid ^ 128 : tid;       // TN: B's blocks on the half of the workgroup that A's leave idle
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

    struct Stage {
        StageA a;
        StageB b;
    };
    auto load_tiles = [&](Stage& r, int k0) __attribute__((always_inline)) {       // (k0 >= K: nothing is read, zeros)
        r.a.load(A, g.lda, g.M, g.K, m0, k0, tid);
        r.b.load(B, g.ldb, g.N, g.K, n0, k0, tid_b);
    };
    auto store_tiles = [&](const Stage& r, int buf) __attribute__((always_inline)) {
        r.a.store(As[buf], tid);
        r.b.store(Bs[buf], tid_b);
    };

    // acc: the sum of a1 b1; lo: the sum of the five correction terms (see the header)
    f32x16 acc[TM][TN], lo[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = lo[i][j][r] = 0.f;

    const int nk = (g.K + kX3BK - 1) / kX3BK;
    const int lr = lane & 31, lk = lane >> 5;
    Stage st0, st1;
    load_tiles(st0, 0);
    store_tiles(st0, 0);
    load_tiles(st0, kX3BK);       // tile 1 -> st0, tile 2 -> st1, tile 3 -> st0, ...
    __syncthreads();
    auto tile_step = [&](int t, Stage& cur, Stage& nxt) __attribute__((always_inline)) {
        // cur holds tile t + 1 (loaded one iteration ago); tile t + 2 goes into nxt
        const int buf = t & 1;
        load_tiles(nxt, (t + 2) * kX3BK);
        // fragments: lane = (row lr, k group lk): eight consecutive k of one row = one 16-byte read per plane; A and B use the same
        // (lane half, element) -> k map, which is all the instruction's sum over k needs
        bf16x8_t af[TM][3], bfr[TN][3];
#pragma unroll
        for (int pl = 0; pl < 3; ++pl) {
#pragma unroll
            for (int i = 0; i < TM; ++i)
                af[i][pl] = __builtin_bit_cast(bf16x8_t, *reinterpret_cast<const uint4*>(&As[buf][pl][lk][4 * swizzle_row(wr * WM + 32 * i + lr)]));
#pragma unroll
            for (int j = 0; j < TN; ++j)
                bfr[j][pl] = __builtin_bit_cast(bf16x8_t, *reinterpret_cast<const uint4*>(&Bs[buf][pl][lk][4 * swizzle_row(wc * WN + 32 * j + lr)]));
        }
        store_tiles(cur, buf ^ 1);       // the other buffer: every wave left it at the barrier that ended the tile before (after the last tile: zeros, unread)
        // the six products, smallest terms first: the five correction terms into `lo`, a1 b1 into `acc`; the TM x TN accumulators take
        // turns inside each term
        constexpr int PA[6] = {2, 0, 1, 1, 0, 0}, PB[6] = {0, 2, 1, 0, 1, 0};
#pragma unroll
        for (int term = 0; term < 5; ++term)
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j)
                    lo[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[i][PA[term]], bfr[j][PB[term]], lo[i][j], 0, 0, 0);
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[i][PA[5]], bfr[j][PB[5]], acc[i][j], 0, 0, 0);
        // issue order: one MFMA, then the VALU / LDS-store work that fits its shadow
#pragma unroll
        for (int m = 0; m < 6 * TM * TN; ++m) {
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
            __builtin_amdgcn_sched_group_barrier(0x002, 6, 0);
            __builtin_amdgcn_sched_group_barrier(0x200, 1, 0);
        }
        __syncthreads();
    };
    // tiles [t0, t1), t0 even
    auto tiles = [&](int t0, int t1) __attribute__((always_inline)) {
        for (int t = t0; t < t1; t += 2) {
            tile_step(t, st0, st1);
            if (t + 1 < t1) tile_step(t + 1, st1, st0);
        }
    };
    if constexpr (A_KM) {
        // two levels, in a loop of its own around the tile loop (a fold predicated inside the tile loop is if-converted: every tile
        // then drains the MFMAs to read the accumulators; gemm_f32_kernel)
        f32x16 tot[TM][TN];
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) tot[i][j][r] = 0.f;
        for (int t0 = 0; t0 < nk; t0 += kX3Fold) {
            tiles(t0, min(t0 + kX3Fold, nk));
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        tot[i][j][r] += acc[i][j][r] + lo[i][j][r];
                        acc[i][j][r] = lo[i][j][r] = 0.f;
                    }
        }
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j) acc[i][j] = tot[i][j];
    } else {
        tiles(0, nk);
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j) acc[i][j] += lo[i][j];
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

std::atomic<int> g_last{-1};       // 3 form + tile (0: 128 x 128, 1: 128 x 64, 2: 64 x 64) of the latest launch; -1: none yet

// Tile by how many workgroups the shape gives, enc_gemm_bf16.hip's rule: 128 x 128 from 256 workgroups on (one per CU), else 128 x 64
// from 256 on, else 64 x 64.  ASPIRE_HIP_GEMM_TILE=128 | 64 pins the first two (tests reach every instantiation with it).
template <int FORM>
int launch_form(const GemmArgs& g, int batch, hipStream_t st) {
    const long long b128 = (long long)((g.M + 127) / 128) * ((g.N + 127) / 128) * batch;
    const long long b12864 = (long long)((g.M + 127) / 128) * ((g.N + 63) / 64) * batch;
    const int ft = tuning().gemm_tile;
    const int tile = ft == 128 ? 0 : ft == 64 ? 1 : (b128 >= 256 && g.N >= 128) ? 0 : b12864 >= 256 ? 1 : 2;
    g_last.store(3 * FORM + tile);
    if (tile == 0)
        hipLaunchKernelGGL((gemm_bf16x3_km_kernel<128, 128, FORM>), dim3((g.N + 127) / 128, (g.M + 127) / 128, batch), dim3(256), 0, st, g);
    else if (tile == 1)
        hipLaunchKernelGGL((gemm_bf16x3_km_kernel<128, 64, FORM>), dim3((g.N + 63) / 64, (g.M + 127) / 128, batch), dim3(256), 0, st, g);
    else
        hipLaunchKernelGGL((gemm_bf16x3_km_kernel<64, 64, FORM>), dim3((g.N + 63) / 64, (g.M + 63) / 64, batch), dim3(256), 0, st, g);
    ASPIRE_LAUNCH_OK();
    return ASPIRE_OK;
}

}  // namespace

int gemm_bf16x3_last() { return g_last.load(); }

int launch_gemm_bf16x3(const GemmArgs& g, int batch, int form, hipStream_t st) {
    if (form == kGemmNT) return launch_gemm(g, batch, false, st);       // the fp32 mode's launch: bf16x3 already wherever K % 16 == 0
    if (g.M <= 0 || g.N <= 0 || batch <= 0) return ASPIRE_OK;
    ASPIRE_REQUIRE(batch <= 65535, ASPIRE_ERR_UNSUPPORTED, "%d matrices in one bf16x3 GEMM launch: the grid's z dimension ends at 65535", batch);
    switch (form) {
        case kGemmBKN: return launch_form<kGemmBKN>(g, batch, st);
        case kGemmTN: return launch_form<kGemmTN>(g, batch, st);
    }
    ASPIRE_REQUIRE(false, ASPIRE_ERR_INVALID_ARG, "unknown GEMM form %d (0 NT, 1 B_KN, 2 TN)", form);
}

}  // namespace aspire

using namespace aspire;

extern "C" int aspire_debug_gemm_bf16x3_f32(const float* A, const float* B, float* C, int64_t M, int64_t N, int64_t K, int64_t lda, int64_t ldb,
                                            int64_t ldc, int form, int64_t batch, int64_t nz2, int64_t sa1, int64_t sa2, int64_t sb1,
                                            int64_t sb2, int64_t sc1, int64_t sc2, float alpha, const float* bias, const float* res, int64_t ldr,
                                            int gelu, void* stream) {
    GemmArgs g;
    bool launch;
    if (int rc = debug_gemm_args(A, B, C, M, N, K, lda, ldb, ldc, form, batch, nz2, sa1, sa2, sb1, sb2, sc1, sc2, alpha, bias, res, ldr, gelu, &g,
                                 &launch))
        return rc;
    if (!launch) return ASPIRE_OK;
    ASPIRE_REQUIRE(form != kGemmNT || K % 4 == 0, ASPIRE_ERR_INVALID_ARG, "the NT form is launch_gemm's: K = %lld is no multiple of 4", (long long)K);
    return launch_gemm_bf16x3(g, (int)batch, form, (hipStream_t)stream);
}
