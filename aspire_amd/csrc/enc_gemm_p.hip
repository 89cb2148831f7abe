// The encoder's GEMMs on pre-split fp16 planes (the P layout: enc_planes.h) -- the product path of every nn.Linear from 1024 token
// rows on -- with the kernel that splits an fp32 matrix into planes, and the device globals of the encoder (the library is built
// without relocatable device code: a device global and the host code that names its symbol share a unit).
//
// Kernels (gemm_p_body is the one loop behind all of them: LDS-DMA ring, three v_mfma_f32_32x32x16_f16 per term)
//   split_planes_kernel      fp32 [R, K] -> P layout (the weights at load time: aspire_bert_prepare_planes)
//   gemm_p_kernel            C = A.B^T (+bias)(+residual) -> fp32, or SWAP: GELU(.) -> the next GEMM's planes; 128 x 128 / 128 x 64 tiles,
//                            rings of 2 .. 4 stages (ASPIRE_HIP_GEMM_RING), PERSIST: resident workgroups walk the tiles (ring 113)
//   gemm_p_w8_kernel         the same on 256 x 128 tiles, eight waves (default for the GELU GEMM and the large QKV GEMM; ASPIRE_HIP_GEMM_TILE=256)
//   gemm_p_qkv_kernel        the QKV projection whose epilogue writes Q, K, V as the fp16 planes flash_attn_p_kernel reads
//   gemm_p_ln_kernel         N = 768 GEMM + bias + residual + LayerNorm in one launch; a row block's column tiles exchange moments and
//                            WAIT for each other, bounded by kLnWaitTicks (g_bert_status, aspire_bert_status)
// Launch rules: launch_gemm_p (tile and ring), launch_gemm_p_qkv, launch_gemm_p_ln, ln_fused_supported; launch_split_planes.
#include <string.h>

#include "enc_planes.h"
#include "enc_types.h"
#include "tuning.h"

namespace aspire {
namespace {

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
int launch_gemm_p_swap(const PGemmArgs& g, hipStream_t st) {
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
}  // namespace

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
namespace {
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
}  // namespace
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

int launch_gemm_p(const PGemmArgs& g, bool swap, hipStream_t st) {
    return swap ? launch_gemm_p_swap<true>(g, st) : launch_gemm_p_swap<false>(g, st);
}

int launch_split_planes(const float* X, int64_t R, int K, void* P, bool weight, int* too_big, hipStream_t st) {
    hipLaunchKernelGGL(split_planes_kernel, dim3((unsigned)((R * (K / 4) + 255) / 256)), dim3(256), 0, st, X, R, K, K, P,
                       weight ? kPWeightScale : 1.0f, too_big);
    ASPIRE_LAUNCH_OK();
    return ASPIRE_OK;
}

}  // namespace aspire

using namespace aspire;

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

#ifdef ASPIRE_PHASE_CLOCK
extern "C" void aspire_debug_gemm_buffer(void* p) {
    long long* q = (long long*)p;
    (void)hipMemcpyToSymbol(HIP_SYMBOL(aspire::g_gdbg), &q, sizeof(q));
}
#endif
