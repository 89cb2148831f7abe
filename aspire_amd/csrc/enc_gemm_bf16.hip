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
// Staging.  The MFMA fragment is eight consecutive k of one row, so the LDS image of a tile is [k group of 8][row][8 bf16], 16 bytes
// per row.  A k-contiguous operand stores its float4 (four k of one row) as one 8-byte half of such a row.  A K-MAJOR operand (a row
// of global memory is a k-slice) is turned IN REGISTERS: a thread loads a 4 k x 4 row block as four float4 along the rows (coalesced:
// eight lanes cover 128 contiguous bytes of a k-slice), and writes each of its four rows' four consecutive k as one 8-byte store into
// the same image -- the scatter route; the fragment reads are then plain 16-byte reads, the same for all three forms.  (The other
// route, storing k-major and reading through the LDS transpose read, needs no register turn but a second read path; NOTES.md.)
// Rows are swizzled, row ^ ((row >> 3) & 3), the same in stores and reads: within an aligned group of four rows a permutation, so a
// fragment read (16 lanes = 16 consecutive rows = 256 bytes) stays conflict free, and the four-row stride of the turned stores
// (rows 4 m + i for eight lanes m) lands on eight distinct 16-byte slots of a 128-byte window instead of two.
//
// Pipeline: 32 k per tile (two MFMA steps), LDS double buffered, the next tile's global loads in flight under this tile's MFMAs,
// converted and stored behind them, one barrier per tile.  Tiles 128 x 128, 128 x 64 and 64 x 64, four waves as 2 x 2.
#include <atomic>

#include "enc_host.h"
#include "tuning.h"

namespace aspire {
namespace {

typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));

// two fp32 -> one dword of two bf16 (low half = the first), round to nearest even
__device__ __forceinline__ uint32_t pack_bf16(float x, float y) {
    typedef __bf16 bf2 __attribute__((ext_vector_type(2)));
    typedef float f2 __attribute__((ext_vector_type(2)));
    const f2 v = {x, y};
    return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, bf2));
}

// p[0 .. 4) where n (<= 0: none) elements from p on are valid; the rest zero.  p is 16-byte aligned.
__device__ __forceinline__ float4 load4_valid(const float* p, int n) {
    if (n >= 4) return *reinterpret_cast<const float4*>(p);
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (n > 0) v.x = p[0];
    if (n > 1) v.y = p[1];
    if (n > 2) v.z = p[2];
    return v;
}

__device__ __forceinline__ int swizzle_row(int r) { return r ^ ((r >> 3) & 3); }

constexpr int kBf16BK = 32;      // k per tile: four groups of eight

// One operand's tile, ROWS x 32 k, from global memory to registers and from registers to its LDS image.  K_MAJOR: the operand is
// [K][ld] with the tile's rows along the contiguous dimension.  `rows` / `K`: the operand's valid extent; r0 / k0: the tile's origin.
template <int ROWS, bool K_MAJOR>
struct StageRegs {
    static constexpr int kPlane = ROWS * 4 + 8;                                    // dwords of one k group: ROWS x 16 bytes + 32 bytes, so that the four groups' stores fall in different quarters of a 128-byte window
    static constexpr int N4 = K_MAJOR ? 4 : ROWS * (kBf16BK / 4) / 256;           // float4 per thread
    static constexpr int kUnits = (ROWS / 4) * (kBf16BK / 4);                      // K_MAJOR: 4 x 4 blocks of the tile (256 or 128)
    float4 v[N4];

    __device__ __forceinline__ void load(const float* X, int ld, int rows, int K, int r0, int k0, int tid) {
        if constexpr (K_MAJOR) {
            // (a 64-row tile has 128 blocks: the upper half of the workgroup stages nothing)
            const bool active = kUnits >= 256 || tid < kUnits;
            const int m4 = ((tid >> 4) % (ROWS / 32)) * 8 + (tid & 7), kq = ((tid >> 4) / (ROWS / 32)) * 2 + ((tid >> 3) & 1);
            const int r = r0 + 4 * m4;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int k = k0 + 4 * kq + j;
                v[j] = load4_valid(X + (size_t)k * ld + r, active && k < K ? rows - r : 0);
            }
        } else {
#pragma unroll
            for (int p = 0; p < N4; ++p) {
                const int idx = tid + 256 * p, row = idx / (kBf16BK / 4), k4 = idx % (kBf16BK / 4);
                const int r = r0 + row, k = k0 + 4 * k4;
                v[p] = load4_valid(X + (size_t)r * ld + k, r < rows ? K - k : 0);
            }
        }
    }
    // S: the buffer's image [4][kPlane]
    __device__ __forceinline__ void store(uint32_t (*S)[kPlane], int tid) const {
        if constexpr (K_MAJOR) {
            if (kUnits < 256 && tid >= kUnits) return;
            const int m4 = ((tid >> 4) % (ROWS / 32)) * 8 + (tid & 7), kq = ((tid >> 4) / (ROWS / 32)) * 2 + ((tid >> 3) & 1);
            uint32_t* base = &S[kq >> 1][2 * (kq & 1)];
            // the turn: k-slice j gives (rows 0, 1) and (rows 2, 3) at k = j as two dwords, rounded where they lie; row i then takes its
            // halves of the four slices' dwords (integer selects: no float leaves its float4)
            uint32_t p01[4], p23[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                p01[q] = pack_bf16(v[q].x, v[q].y);
                p23[q] = pack_bf16(v[q].z, v[q].w);
            }
            auto lo = [](uint32_t a, uint32_t b) { return (a & 0xffffu) | (b << 16); };
            auto hi = [](uint32_t a, uint32_t b) { return (a >> 16) | (b & 0xffff0000u); };
            *reinterpret_cast<uint2*>(base + 4 * swizzle_row(4 * m4 + 0)) = make_uint2(lo(p01[0], p01[1]), lo(p01[2], p01[3]));
            *reinterpret_cast<uint2*>(base + 4 * swizzle_row(4 * m4 + 1)) = make_uint2(hi(p01[0], p01[1]), hi(p01[2], p01[3]));
            *reinterpret_cast<uint2*>(base + 4 * swizzle_row(4 * m4 + 2)) = make_uint2(lo(p23[0], p23[1]), lo(p23[2], p23[3]));
            *reinterpret_cast<uint2*>(base + 4 * swizzle_row(4 * m4 + 3)) = make_uint2(hi(p23[0], p23[1]), hi(p23[2], p23[3]));
        } else {
#pragma unroll
            for (int p = 0; p < N4; ++p) {
                const int idx = tid + 256 * p, row = idx / (kBf16BK / 4), k4 = idx % (kBf16BK / 4);
                *reinterpret_cast<uint2*>(&S[k4 >> 1][4 * swizzle_row(row) + 2 * (k4 & 1)]) =
                    make_uint2(pack_bf16(v[p].x, v[p].y), pack_bf16(v[p].z, v[p].w));
            }
        }
    }
};

template <int BM, int BN, int FORM>
__global__ void __launch_bounds__(256) gemm_bf16_kernel(GemmArgs g) {
    constexpr bool A_KM = FORM == kGemmTN, B_KM = FORM != kGemmNT;
    constexpr int WAVES_N = 2;
    constexpr int WM = BM / 2, WN = BN / 2, TM = WM / 32, TN = WN / 32;
    static_assert(WM % 32 == 0 && WN % 32 == 0, "tile / wave layout");
    using StageA = StageRegs<BM, A_KM>;
    using StageB = StageRegs<BN, B_KM>;
    __shared__ __attribute__((aligned(16))) uint32_t As[2][4][StageA::kPlane];
    __shared__ __attribute__((aligned(16))) uint32_t Bs[2][4][StageB::kPlane];

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
                af[i] = __builtin_bit_cast(bf16x8_t, *reinterpret_cast<const uint4*>(&As[buf][2 * s + lk][4 * swizzle_row(wr * WM + 32 * i + lr)]));
#pragma unroll
            for (int j = 0; j < TN; ++j)
                bfr[j] = __builtin_bit_cast(bf16x8_t, *reinterpret_cast<const uint4*>(&Bs[buf][2 * s + lk][4 * swizzle_row(wc * WN + 32 * j + lr)]));
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
    ASPIRE_REQUIRE(A && B && C, ASPIRE_ERR_INVALID_ARG, "null pointer (A / B / C)");
    ASPIRE_REQUIRE(M >= 0 && N >= 0 && K >= 0 && batch >= 0, ASPIRE_ERR_INVALID_ARG, "negative size (M %lld N %lld K %lld batch %lld)",
                   (long long)M, (long long)N, (long long)K, (long long)batch);
    ASPIRE_REQUIRE(form == kGemmNT || form == kGemmBKN || form == kGemmTN, ASPIRE_ERR_INVALID_ARG, "unknown GEMM form %d (0 NT, 1 B_KN, 2 TN)",
                   form);
    ASPIRE_REQUIRE(nz2 >= 1, ASPIRE_ERR_INVALID_ARG, "nz2 = %lld: the inner batch count is at least 1", (long long)nz2);
    // what each operand's rows must span, and the float4 rule of the fp32 forms
    const int64_t a_cols = form == kGemmTN ? M : K, b_cols = form == kGemmNT ? K : N;
    ASPIRE_REQUIRE(lda >= a_cols && ldb >= b_cols && ldc >= N && (!res || ldr >= N), ASPIRE_ERR_INVALID_ARG,
                   "a leading dimension is shorter than its row (lda %lld ldb %lld ldc %lld ldr %lld)", (long long)lda, (long long)ldb,
                   (long long)ldc, (long long)ldr);
    ASPIRE_REQUIRE(lda % 4 == 0 && ldb % 4 == 0 && (sa1 | sa2 | sb1 | sb2) % 4 == 0 && (((uintptr_t)A | (uintptr_t)B) & 15) == 0,
                   ASPIRE_ERR_INVALID_ARG, "A and B are read as float4: 16-byte aligned bases, lda / ldb / batch strides multiples of 4");
    ASPIRE_REQUIRE(M < (1 << 30) && N < (1 << 30) && K < (1 << 30) && lda < (1 << 30) && ldb < (1 << 30) && ldc < (1 << 30) && ldr < (1 << 30) &&
                       batch <= 65535,
                   ASPIRE_ERR_UNSUPPORTED, "a size beyond the kernel's 32-bit indices (or more than 65535 matrices)");
    if (M == 0 || N == 0 || K == 0 || batch == 0) return ASPIRE_OK;
    GemmArgs g{};
    g.A = A; g.B = B; g.C = C; g.bias = bias; g.res = res;
    g.M = (int)M; g.N = (int)N; g.K = (int)K; g.lda = (int)lda; g.ldb = (int)ldb; g.ldc = (int)ldc; g.ldr = (int)ldr;
    g.nz2 = (int)nz2; g.sa1 = sa1; g.sa2 = sa2; g.sb1 = sb1; g.sb2 = sb2; g.sc1 = sc1; g.sc2 = sc2;
    g.alpha = alpha; g.gelu = gelu ? 1 : 0;
    return launch_gemm_bf16(g, (int)batch, form, (hipStream_t)stream);
}
