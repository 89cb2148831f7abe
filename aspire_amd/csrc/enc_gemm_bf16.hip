// The training encoder's matrix products in bf16 (the opt-in mode ASPIRE_MATMUL_BF16): one GEMM on v_mfma_f32_32x32x16_bf16 that takes
// the GemmArgs of launch_gemm / launch_gemm_tn -- batched and strided, alpha, bias, GELU and residual epilogues in fp32, fp32 output.
//
// The arithmetic of the mode, and nothing else:
//   * every operand element is rounded to bf16 ONCE, round to nearest even, when its tile is staged from the fp32 tensor into LDS
//     (v_cvt_pk_bf16_f32: torch.Tensor.to(torch.bfloat16)'s values -- +-0 and ties as torch gives them, +-inf kept, NaN stays NaN, a
//     magnitude that rounds past bf16's largest finite becomes inf);
//   * a product of two bf16 values is exact in fp32;
//   * sums are the MFMA's fp32 accumulators in k order, ONE level in every form: the TN form does not keep gemm_f32_kernel's second
//     accumulator set (there it bounds the drift of a running fp32 sum over thousands of token rows, ~ rows x 2^-24; here each operand
//     already carries 2^-9 of rounding, three orders of magnitude above that drift at 5 000 rows);
//   * the epilogue (alpha, bias, GELU, residual) is fp32;
//   * no atomics, one writer per output element: the same bits on every run.
//
// Forms (enc_host.h: kGemmNT / kGemmBKN / kGemmTN)
//   NT    A [M, K], B [N, K], both k-contiguous     nn.Linear forwards, Q K^T, dP = dctx V^T
//   B_KN  A [M, K], B [K, N] n-contiguous            P V, every dX = dY W, dQ = dS K
//   TN    A [K, M], B [K, N], both k-major           every dW = dY^T X, dV = P^T dctx, dK = dS^T Q
// Any M, N, K: tails are zero-filled when a tile is staged (a partial float4 is read element by element, never past the operand's
// valid extent); lda / ldb multiples of 4 and 16-byte aligned bases, as the fp32 forms ask.
//
// Staging: StageRegs of enc_stage.h with one plane (the loads, the register turn of a k-major operand, the swizzled LDS image).
//
// Pipeline: 32 k per tile (two MFMA steps), LDS double buffered, the next tile's global loads in flight under this tile's MFMAs,
// converted and stored behind them, one barrier per tile.  Tiles 128 x 128, 128 x 64 and 64 x 64, four waves as 2 x 2.
#include <atomic>

#include "enc_host.h"
#include "enc_stage.h"
#include "tuning.h"

namespace aspire {
namespace {

constexpr int kBf16BK = 32;      // k per tile: four groups of eight

template <int BM, int BN, int FORM>
__global__ void __launch_bounds__(256) gemm_bf16_kernel(GemmArgs g) {
    constexpr bool A_KM = FORM == kGemmTN, B_KM = FORM != kGemmNT;
    constexpr int WAVES_N = 2;
    constexpr int WM = BM / 2, WN = BN / 2, TM = WM / 32, TN = WN / 32;
    static_assert(WM % 32 == 0 && WN % 32 == 0, "tile / wave layout");
    using StageA = StageRegs<BM, A_KM, kBf16BK, 1>;
    using StageB = StageRegs<BN, B_KM, kBf16BK, 1>;
    __shared__ __attribute__((aligned(16))) uint32_t As[2][1][4][StageA::kPlane];
    __shared__ __attribute__((aligned(16))) uint32_t Bs[2][1][4][StageB::kPlane];

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

    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    StageA ra;
    StageB rb;
    const int nk = (g.K + kBf16BK - 1) / kBf16BK;
    ra.load(A, g.lda, g.M, g.K, m0, 0, tid);
    rb.load(B, g.ldb, g.N, g.K, n0, 0, tid);
    ra.store(As[0], tid);
    rb.store(Bs[0], tid);
    __syncthreads();
    const int lr = lane & 31, lk = lane >> 5;
    for (int t = 0; t < nk; ++t) {
        const int buf = t & 1;
        if (t + 1 < nk) {       // in flight under the MFMAs below
            ra.load(A, g.lda, g.M, g.K, m0, (t + 1) * kBf16BK, tid);
            rb.load(B, g.ldb, g.N, g.K, n0, (t + 1) * kBf16BK, tid);
        }
        // fragments: lane = (row lr, k group lk of the step): eight consecutive k of one row = one 16-byte read; A and B use the same
        // (lane half, element) -> k map, which is all the instruction's sum over k needs
#pragma unroll
        for (int s = 0; s < kBf16BK / 16; ++s) {
            bf16x8_t af[TM], bfr[TN];
#pragma unroll
            for (int i = 0; i < TM; ++i)
                af[i] = __builtin_bit_cast(bf16x8_t, *reinterpret_cast<const uint4*>(&As[buf][0][2 * s + lk][4 * swizzle_row(wr * WM + 32 * i + lr)]));
#pragma unroll
            for (int j = 0; j < TN; ++j)
                bfr[j] = __builtin_bit_cast(bf16x8_t, *reinterpret_cast<const uint4*>(&Bs[buf][0][2 * s + lk][4 * swizzle_row(wc * WN + 32 * j + lr)]));
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[i], bfr[j], acc[i][j], 0, 0, 0);
        }
        if (t + 1 < nk) {       // the other buffer: every wave left it at the barrier that ended the tile before
            ra.store(As[buf ^ 1], tid);
            rb.store(Bs[buf ^ 1], tid);
        }
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

std::atomic<int> g_last{-1};       // 3 form + tile (0: 128 x 128, 1: 128 x 64, 2: 64 x 64) of the latest launch; -1: none yet

// Tile by how many workgroups the shape gives, the fp32 forms' rule of thumb at this kernel's footprint (232 registers and 33 KB of LDS
// at 128 x 128: two workgroups fit a CU, one per CU is the least worth having): 128 x 128 from 256 workgroups on, else 128 x 64 from
// 256 on, else 64 x 64.  ASPIRE_HIP_GEMM_TILE=128 | 64 pins the first two (tests reach every instantiation with it).
template <int FORM>
int launch_form(const GemmArgs& g, int batch, hipStream_t st) {
    const long long b128 = (long long)((g.M + 127) / 128) * ((g.N + 127) / 128) * batch;
    const long long b12864 = (long long)((g.M + 127) / 128) * ((g.N + 63) / 64) * batch;
    const int ft = tuning().gemm_tile;
    const int tile = ft == 128 ? 0 : ft == 64 ? 1 : (b128 >= 256 && g.N >= 128) ? 0 : b12864 >= 256 ? 1 : 2;
    g_last.store(3 * FORM + tile);
    if (tile == 0)
        hipLaunchKernelGGL((gemm_bf16_kernel<128, 128, FORM>), dim3((g.N + 127) / 128, (g.M + 127) / 128, batch), dim3(256), 0, st, g);
    else if (tile == 1)
        hipLaunchKernelGGL((gemm_bf16_kernel<128, 64, FORM>), dim3((g.N + 63) / 64, (g.M + 127) / 128, batch), dim3(256), 0, st, g);
    else
        hipLaunchKernelGGL((gemm_bf16_kernel<64, 64, FORM>), dim3((g.N + 63) / 64, (g.M + 63) / 64, batch), dim3(256), 0, st, g);
    ASPIRE_LAUNCH_OK();
    return ASPIRE_OK;
}

}  // namespace

int gemm_bf16_last() { return g_last.load(); }

int launch_gemm_bf16(const GemmArgs& g, int batch, int form, hipStream_t st) {
    if (g.M <= 0 || g.N <= 0 || batch <= 0) return ASPIRE_OK;
    ASPIRE_REQUIRE(batch <= 65535, ASPIRE_ERR_UNSUPPORTED, "%d matrices in one bf16 GEMM launch: the grid's z dimension ends at 65535", batch);
    switch (form) {
        case kGemmNT: return launch_form<kGemmNT>(g, batch, st);
        case kGemmBKN: return launch_form<kGemmBKN>(g, batch, st);
        case kGemmTN: return launch_form<kGemmTN>(g, batch, st);
    }
    ASPIRE_REQUIRE(false, ASPIRE_ERR_INVALID_ARG, "unknown GEMM form %d (0 NT, 1 B_KN, 2 TN)", form);
}

}  // namespace aspire

using namespace aspire;

extern "C" int aspire_debug_gemm_bf16_f32(const float* A, const float* B, float* C, int64_t M, int64_t N, int64_t K, int64_t lda, int64_t ldb,
                                          int64_t ldc, int form, int64_t batch, int64_t nz2, int64_t sa1, int64_t sa2, int64_t sb1, int64_t sb2,
                                          int64_t sc1, int64_t sc2, float alpha, const float* bias, const float* res, int64_t ldr, int gelu,
                                          void* stream) {
    GemmArgs g;
    bool launch;
    if (int rc = debug_gemm_args(A, B, C, M, N, K, lda, ldb, ldc, form, batch, nz2, sa1, sa2, sb1, sb2, sc1, sc2, alpha, bias, res, ldr, gelu, &g,
                                 &launch))
        return rc;
    if (!launch) return ASPIRE_OK;
    return launch_gemm_bf16(g, (int)batch, form, (hipStream_t)stream);
}
