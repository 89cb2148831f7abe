// The GEMMs of the inference encoder's opt-in fp16 matmul mode (ASPIRE_MATMUL_FP16) on single-plane fp16 operands (the H layout:
// enc_hplane.h), with the kernels that bring fp32 rows into that layout.  Every operand element was rounded to fp16 once, a product
// of two fp16 values is exact in fp32, the sums are the matrix cores' fp32 accumulators in a fixed order, the epilogues are fp32.
// No atomics, no in-kernel waits, no device globals: every output element has one writer, the same bits on every run and stream.
//
// Kernels
//   split_h_kernel        fp32 [R, K] (row stride ld) -> H layout (the weights at load time: aspire_bert_prepare_hplanes; the embedding
//                         LayerNorm's output and the attention context per forward)
//   layernorm_h_kernel    y = LN(x) * gamma + beta as layernorm_kernel (enc_rows.hip) forms it, the fp32 row and its H copy in one pass
//   gemm_h_kernel         C = A.B^T: 128 x 128 tiles of four 64 x 64 waves (128 x 64 for column tails and short launches), a three-stage
//                         LDS ring filled by LDS-DMA two stages ahead; a stage is one 32-wide k block = two MFMA k steps: per stage and
//                         wave 8 fragment reads and 8 v_mfma_f32_32x32x16_f16 (one product per term; gemm_p_kernel: 12 per 16 k).
//                         Epilogue (a): + bias (+ fp32 residual) -> fp32, coalesced 128-byte stores; (b), operands swapped:
//                         GELU(acc + bias) -> the H layout of the next GEMM's A operand
// Launch rules: launch_gemm_h, launch_split_h, launch_layernorm_h.
#include "enc_hplane.h"
#include "enc_types.h"
#include "tuning.h"

namespace aspire {
namespace {

// *too_big (optional) is raised when an element leaves fp16's range (|scale x| > 65504, or not finite)
__global__ void __launch_bounds__(256) split_h_kernel(const float* __restrict__ X, int64_t R, int K, int64_t ld, void* __restrict__ H,
                                                      float scale, int* __restrict__ too_big) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int k4 = K / 4;
    if (idx >= R * k4) return;
    const int64_t r = idx / k4;
    const int k = (int)(idx % k4) * 4;
    const float4 v = *reinterpret_cast<const float4*>(X + r * ld + k);
    h_store4(H, R, r, k, scale * v.x, scale * v.y, scale * v.z, scale * v.w);
    if (too_big && !(fmaxf(fmaxf(fabsf(v.x), fabsf(v.y)), fmaxf(fabsf(v.z), fabsf(v.w))) * scale <= 65504.f)) *too_big = 1;
}

// One wave per row of 768, four rows per workgroup: lane holds 3 float4 (d = 4 lane + 256 c); the moments as layernorm_kernel's
// (mean first, then the sum of squared deviations).  yh (optional): the row's H copy, the A operand of the GEMM that reads it
__global__ void __launch_bounds__(256) layernorm_h_kernel(const float* __restrict__ x, const float* __restrict__ gamma,
                                                          const float* __restrict__ beta, float eps, float* __restrict__ y, int64_t rows,
                                                          void* __restrict__ yh) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    float4 v[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c] = *reinterpret_cast<const float4*>(x + row * kD + 4 * lane + 256 * c);
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
        *reinterpret_cast<float4*>(y + row * kD + d) = o;
        if (yh) h_store4(yh, rows, row, d, o.x, o.y, o.z, o.w);
    }
}

// One 16-byte-per-lane LDS-DMA of a k block's pieces, as enc_gemm_p.hip's glds_kblock (duplicated here: that unit's kernels keep their
// bytes): 64 lanes x 16 B from global bytes [base + IMM + voff(lane)] to LDS bytes [lds_dst + IMM, .. + 1024); a uniform 64-bit base in
// SGPRs plus a per-lane 32-bit offset that never changes.  hipcc does not count this load: the caller waits with s_waitcnt vmcnt(N)
// itself.  M0 is compiler-reserved: saved and restored inside the statement.  Two 1 KB pieces of A, TWO_B ? two : one of B.
template <bool TWO_B>
__device__ __forceinline__ void glds_hblock(uint64_t a_base, uint64_t b_base, uint32_t voff, uint32_t a_dst, uint32_t b_dst) {
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

constexpr int kHRing = 3;       // stages of one k block: 48 KB at 128 x 128, three workgroups per CU

// C = A . B^T on 128 x BN tiles, four waves of 64 x (BN / 2), modelled on gemm_p_body's non-persistent form without the LayerNorm
// epilogue.  Order of a step: wait for the own pieces of stage t (s_waitcnt vmcnt(kPerWave x the younger stages in flight)), barrier
// (everybody's pieces of stage t have landed AND everybody has read stage t - 1, whose slot is free now), issue stage t + 2 into that
// slot, read the 8 fragments of both k steps, multiply.
// Tail rows (m >= M) of the last row tile read whatever lies behind the matrix (the next k block's rows, the kPPadRows of slack): a
// row of A meets only its own row of C, which is never written.
// SWAP: the MFMA's operands exchanged -- accumulator registers run along n, the lane is a row m -- for the epilogue that writes
// GELU(.) straight into the H layout [M, N] of the next GEMM's A operand (the lane pair exchanges register groups: a lane then owns 8
// consecutive columns = one 16-byte piece); otherwise registers run along m, lanes along n: 128-byte coalesced fp32 stores.
template <int BN, bool SWAP>
__device__ __forceinline__ void gemm_h_body(const HGemmArgs& g) {
    constexpr int NS = kHRing;
    constexpr int TN = BN / 64;                             // 32-column blocks per wave
    constexpr int kATile = kHTile, kBTile = BN * kHRowBytes;
    constexpr int kStage = kATile + kBTile;                 // [A rows of the k block][B rows of the k block]
    constexpr int kBPerWave = kBTile / (32 * 128);          // 1 KB pieces per wave and k block: 2 (128 x 128) or 1
    constexpr int kPerWave = 2 + kBPerWave;                 // LDS-DMA instructions per wave and stage
    extern __shared__ __attribute__((aligned(16))) unsigned char h_smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wave >> 1, wc = wave & 1, lr = lane & 31, lk = lane >> 5;
    // XCD-aware tile order, as gemm_p_kernel: XCD x = workgroup id mod 8 owns a contiguous run of the tile sequence
    const uint32_t gx = gridDim.x, nb = gx * gridDim.y;
    const uint32_t wg = blockIdx.x + gridDim.x * blockIdx.y;
    const uint32_t xcd = wg & 7, q8 = nb >> 3, r8 = nb & 7;
    const uint32_t tile = xcd * q8 + (xcd < r8 ? xcd : r8) + (wg >> 3);
    const uint32_t bx = tile % gx, by = tile / gx;
    const int m0 = (int)by * 128, n0 = g.n_off + (int)bx * BN;
    const int nk = g.K / kHBlockK;
    const uint32_t lds0 = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) unsigned char*)h_smem;
    // per k block wave w moves pieces 2 w, 2 w + 1 (1 KB = 16 rows each) of the A rows and pieces 2 w, 2 w + 1 (BN = 64: piece w) of B's
    const uint64_t a_src = (uint64_t)(uintptr_t)g.Ah + (2 * wave) * 1024 + (uint64_t)m0 * kHRowBytes;
    const uint64_t b_src = (uint64_t)(uintptr_t)g.Bh + (kBPerWave * wave) * 1024 + (uint64_t)n0 * kHRowBytes;
    const uint64_t a_step = (uint64_t)g.M * kHRowBytes, b_step = (uint64_t)g.N * kHRowBytes;
    const uint32_t lane16 = lane * 16;
    auto issue = [&](int slot, int t) {
        const uint32_t dst = lds0 + slot * kStage;
        glds_hblock<kBPerWave == 2>(a_src + (uint64_t)t * a_step, b_src + (uint64_t)t * b_step, lane16, dst + (2 * wave) * 1024,
                                    dst + kATile + (kBPerWave * wave) * 1024);
    };
    // fragment of this lane's row for MFMA k step s: piece (2 s + lk) ^ ((row >> 2) & 3); the row's bits 2..3 are lr's (tiles and wave
    // tiles start on multiples of 32)
    const uint32_t frag0 = 16 * (lk ^ ((lr >> 2) & 3));
    const unsigned char* a_rd = h_smem + (wr * 64 + lr) * kHRowBytes;
    const unsigned char* b_rd = h_smem + kATile + (wc * 32 * TN + lr) * kHRowBytes;

    f32x16 acc[2][TN];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

#pragma unroll
    for (int s = 0; s < NS - 1; ++s)
        if (s < nk) issue(s, s);
    struct Frags {
        f16x8_t a[2][2], b[TN][2];       // [block][k step]
    };
    auto read_frags = [&](Frags& f, int slot) {
#pragma unroll
        for (int s = 0; s < 2; ++s) {          // the first k step's fragments first: its products start while the second's land
            const uint32_t fo = frag0 ^ (32 * s);
#pragma unroll
            for (int i = 0; i < 2; ++i)
                f.a[i][s] = __builtin_bit_cast(f16x8_t, *reinterpret_cast<const uint4*>(a_rd + slot * kStage + i * 32 * kHRowBytes + fo));
#pragma unroll
            for (int j = 0; j < TN; ++j)
                f.b[j][s] = __builtin_bit_cast(f16x8_t, *reinterpret_cast<const uint4*>(b_rd + slot * kStage + j * 32 * kHRowBytes + fo));
        }
    };
    auto mma = [&](const Frags& f) {
#pragma unroll
        for (int s = 0; s < 2; ++s)
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j) {
                    if constexpr (SWAP)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(f.b[j][s], f.a[i][s], acc[i][j], 0, 0, 0);
                    else
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(f.a[i][s], f.b[j][s], acc[i][j], 0, 0, 0);
                }
    };
    static_assert(NS == 3 && kPerWave < 64, "ring depth");
    auto step = [&](int t, int slot) {
        // the own pieces of stage t: everything but the one younger stage's pieces (none at the end of the loop).  lgkmcnt(0): this
        // wave's fragment reads of the previous stage are done before anybody may refill that slot.
        if (nk - 1 - t >= 1) asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(kPerWave) : "memory");
        else asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        if (t + NS - 1 < nk) issue((slot + NS - 1) % NS, t + NS - 1);
        Frags f;
        read_frags(f, slot);
        // all 8 fragment reads go out before the first MFMA
        __builtin_amdgcn_sched_barrier(0);
        mma(f);
    };
    for (int t = 0; t < nk; t += NS) {
#pragma unroll
        for (int s = 0; s < NS; ++s)
            if (t + s < nk) step(t + s, s);
    }

    constexpr float kUnscale = 1.0f / kPWeightScale;
    if constexpr (!SWAP) {
        // C/D layout of the 32 x 32 MFMA: col = lane & 31 (n), row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5) (m): a store instruction writes
        // two full 128-byte lines.  Whole tiles take the branch-free form: the residual's 16 loads of a block go out together, the 16
        // stores follow back to back; the last row tile checks every row
        float bias_n[TN];
#pragma unroll
        for (int j = 0; j < TN; ++j) bias_n[j] = 0.f;
        if (g.bias) {
#pragma unroll
            for (int j = 0; j < TN; ++j) bias_n[j] = g.bias[n0 + wc * 32 * TN + 32 * j + lr];
        }
#pragma unroll
        for (int j = 0; j < TN; ++j) asm volatile("" : "+v"(bias_n[j]));       // consumed in front of the first store: one wait
        const bool whole = m0 + 128 <= g.M;
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
                    if (g.res) {
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
                    if (g.res) v += g.res[(size_t)m * g.ldr + n];
                    g.C[(size_t)m * g.ldc + n] = v;
                }
            }
    } else {
        // swapped: col = lane & 31 is the row m, the registers run along n in groups of 4 consecutive, the lane pair (lk) interleaved:
        // n = 8 g + 4 lk + e.  GELU in the accumulators' own layout, then one v_permlane32_swap per register pair: lane half lk holds
        // columns 16 t + 8 lk + 0 .. 7 of a 32-column block = one whole 16-byte piece of the H layout [M, N] (k dimension = n)
        float4 bias_m[TN][4];
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int q4 = 0; q4 < 4; ++q4) bias_m[j][q4] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (g.bias) {
#pragma unroll
            for (int j = 0; j < TN; ++j)
#pragma unroll
                for (int q4 = 0; q4 < 4; ++q4) bias_m[j][q4] = *reinterpret_cast<const float4*>(g.bias + n0 + wc * 32 * TN + 32 * j + 8 * q4 + 4 * lk);
        }
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int q4 = 0; q4 < 4; ++q4)
                asm volatile("" : "+v"(bias_m[j][q4].x), "+v"(bias_m[j][q4].y), "+v"(bias_m[j][q4].z), "+v"(bias_m[j][q4].w));
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
                        // (scalars first, both ways: a bit_cast applied to a vector ELEMENT reads element 0 with this clang)
                        const float fa = gelu_erf(fmaf(acc[i][j][8 * t + e], kUnscale, b_a)), fb = gelu_erf(fmaf(acc[i][j][8 * t + 4 + e], kUnscale, b_b));
                        auto r = __builtin_amdgcn_permlane32_swap(__builtin_bit_cast(int, fa), __builtin_bit_cast(int, fb), false, false);
                        const int x0 = r[0], x1 = r[1];
                        o[e] = __builtin_bit_cast(float, x0);
                        o[4 + e] = __builtin_bit_cast(float, x1);
                    }
                    if (m < g.M) h_store8_at(g.Ch, h_slot8((uint32_t)g.M, (uint32_t)m, (uint32_t)(n0 + wc * 32 * TN + 32 * j + 16 * t + 8 * lk)), o);
                }
        }
    }
}

template <int BN, bool SWAP>
__global__ void __launch_bounds__(256, 2) gemm_h_kernel(HGemmArgs g) {
    gemm_h_body<BN, SWAP>(g);
}

template <int BN, bool SWAP>
int launch_gemm_h_bn(HGemmArgs g, int n_off, int col_tiles, hipStream_t st) {
    constexpr int lds = kHRing * (kHTile + BN * kHRowBytes);
    static hipError_t raised = hipFuncSetAttribute(reinterpret_cast<const void*>(gemm_h_kernel<BN, SWAP>), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    ASPIRE_HIP_OK(raised);
    g.n_off = n_off;
    hipLaunchKernelGGL((gemm_h_kernel<BN, SWAP>), dim3(col_tiles, (g.M + 127) / 128), dim3(256), lds, st, g);
    ASPIRE_LAUNCH_OK();
    return ASPIRE_OK;
}

template <bool SWAP>
int launch_gemm_h_swap(const HGemmArgs& g, hipStream_t st) {
    // 128 x 128 tiles; 128 x 64 ones for a column tail (N % 128 == 64) and, as launch_gemm_p chooses, for the whole of a short-k GEMM
    // whose 128-wide tiles could not give every resident workgroup slot (three per CU) a tile.  ASPIRE_HIP_GEMM_TILE=128 | 64 pins the
    // width (tests: every shape on both)
    const long long slots = 768, rows = (g.M + 127) / 128, n128 = g.N / 128;
    int c1 = (int)n128;
    if (tuning().gemm_tile == 64 || (tuning().gemm_tile != 128 && rows * n128 < slots && g.K <= 1024)) c1 = 0;
    if (c1 > 0)
        if (int rc = launch_gemm_h_bn<128, SWAP>(g, 0, c1, st)) return rc;
    if (c1 * 128 < g.N)
        if (int rc = launch_gemm_h_bn<64, SWAP>(g, c1 * 128, (g.N - c1 * 128) / 64, st)) return rc;
    return ASPIRE_OK;
}

}  // namespace

int launch_gemm_h(const HGemmArgs& g, bool gelu_h, hipStream_t st) {
    ASPIRE_REQUIRE(g.M >= 1 && g.N > 0 && g.N % 64 == 0 && g.K > 0 && g.K % kHBlockK == 0, ASPIRE_ERR_UNSUPPORTED,
                   "H-layout GEMM needs M >= 1, N %% 64 == 0 and K %% 32 == 0 (M %d, N %d, K %d)", g.M, g.N, g.K);
    ASPIRE_REQUIRE(g.Ah && g.Bh && (gelu_h ? g.Ch != nullptr : g.C != nullptr), ASPIRE_ERR_INVALID_ARG, "null pointer");
    // the H layout's slots are 32-bit byte offsets (h_slot8), and a k block's rows are addressed from a 64-bit base: the output is the widest
    ASPIRE_REQUIRE(!gelu_h || (uint64_t)g.M * (uint64_t)g.N * 2 < (1ull << 32), ASPIRE_ERR_UNSUPPORTED,
                   "%d x %d: the fp16-plane layout addresses < 4 GB per operand (split the batch)", g.M, g.N);
    return gelu_h ? launch_gemm_h_swap<true>(g, st) : launch_gemm_h_swap<false>(g, st);
}

int launch_split_h(const float* X, int64_t R, int K, int64_t ld, void* H, bool weight, int* too_big, hipStream_t st) {
    hipLaunchKernelGGL(split_h_kernel, dim3((unsigned)((R * (K / 4) + 255) / 256)), dim3(256), 0, st, X, R, K, ld, H,
                       weight ? kPWeightScale : 1.0f, too_big);
    ASPIRE_LAUNCH_OK();
    return ASPIRE_OK;
}

int launch_layernorm_h(const float* x, const float* gamma, const float* beta, float eps, float* y, int64_t rows, void* yh, hipStream_t st) {
    hipLaunchKernelGGL(layernorm_h_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, st, x, gamma, beta, eps, y, rows, yh);
    ASPIRE_LAUNCH_OK();
    return ASPIRE_OK;
}

}  // namespace aspire

using namespace aspire;

// Debug entries of the H layout (tests/test_gpu_gemm_hplane.py, tools): a buffer's size, one operand into the layout (weight != 0: the
// B side, scaled by 64), and one product.  epilogue 0: C [M, N] fp32 = A.B^T / 64 (+ bias) (+ res [M, N]); 1: Ch [M, N] H layout =
// GELU(A.B^T / 64 + bias)
extern "C" size_t aspire_debug_hplane_bytes(int64_t R, int64_t K) { return R > 0 && K > 0 ? h_bytes(R, K) : 0; }

extern "C" int aspire_debug_split_hplane(const float* X, int64_t R, int64_t K, void* H, int weight, void* stream) {
    ASPIRE_REQUIRE(X && H, ASPIRE_ERR_INVALID_ARG, "null pointer");
    ASPIRE_REQUIRE(R >= 1 && K >= 32 && K % 32 == 0 && K <= (1 << 20), ASPIRE_ERR_UNSUPPORTED, "H layout: R >= 1 and K %% 32 == 0 (R %lld, K %lld)",
                   (long long)R, (long long)K);
    ASPIRE_REQUIRE((uint64_t)R * (uint64_t)K / 4 < (1ull << 39), ASPIRE_ERR_UNSUPPORTED, "matrix too large");
    return launch_split_h(X, R, (int)K, K, H, weight != 0, nullptr, (hipStream_t)stream);
}

extern "C" int aspire_debug_gemm_hplane(const void* Ah, const void* Bh, float* C, void* Ch, const float* bias, const float* res, int64_t M,
                                        int64_t N, int64_t K, int epilogue, void* stream) {
    ASPIRE_REQUIRE(epilogue == 0 || epilogue == 1, ASPIRE_ERR_INVALID_ARG, "epilogue %d: 0 (fp32 out) or 1 (GELU -> H layout)", epilogue);
    ASPIRE_REQUIRE(M >= 1 && N >= 1 && K >= 1 && M < (1 << 24) && N < (1 << 24) && K < (1 << 24), ASPIRE_ERR_INVALID_ARG,
                   "sizes out of range (M %lld, N %lld, K %lld)", (long long)M, (long long)N, (long long)K);
    ASPIRE_REQUIRE(!(epilogue == 1 && res), ASPIRE_ERR_INVALID_ARG, "the GELU epilogue takes no residual");
    HGemmArgs g{Ah, Bh, C, Ch, bias, res, (int)M, (int)N, (int)K, (int)N, (int)N, 0};
    return launch_gemm_h(g, epilogue == 1, (hipStream_t)stream);
}
