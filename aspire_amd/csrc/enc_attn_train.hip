// The training encoder's fused attention (the opt-in mode ASPIRE_ATTENTION_FLASH, with ASPIRE_MATMUL_BF16 only): the forward keeps two
// row statistics per (document, head, query) instead of the [L, L] probabilities, the backward forms the probabilities again.
//
// Kernels (gfx950; fp32 in and out, v_mfma_f32_32x32x16_bf16, fp32 accumulators, soft-max and epilogues)
//   flash_train_fwd_kernel   one workgroup per (document, head, 128 queries): ctx = drop(softmax(Q K^T / 8 + mask)) V and, per query,
//                            (m, l) = the row maximum of the scores in log2 units and the row sum of exp2(s - m), UNdropped
//   flash_train_d_kernel     D[b, h, i] = sum_d bf16(dctx) . ctx over the head's 64 columns (= rowsum(dP . P), with dropout as well:
//                            ctx is the product with the dropped P), fp32 sums
//   flash_train_dkv_kernel   one workgroup per (document, head, 128 keys) walks the query tiles: dV = P_drop^T dctx,
//                            dK = dS^T Q / 8, dS = P . (keep scale (dctx V^T) - D)
//   flash_train_dq_kernel    one workgroup per (document, head, 128 queries) walks the key tiles: dQ = dS K / 8
// No atomics, no wait on another workgroup; every element of ctx, stats and dqkv [M, 2304] has one writer and every sum a fixed order:
// the same bits on every run.
//
// The arithmetic, and nothing else: Q, K, V, dctx are rounded to bf16 once (round to nearest even: pack_bf16 of enc_stage.h) as their
// tiles are staged from the fp32 tensors; scores are fp32; the soft-max is online with exp2; the forward rounds the UNNORMALISED
// probability exp2(s - m_run), times keep . scale where the site drops, to bf16 on its way into the second product and divides by the
// row sum in fp32 at the end; the backward rounds P_drop = keep scale exp2(s - m) / l and dS to bf16 as they enter their products; the
// factor 1 / 8 of dQ and dK is an fp32 epilogue.
//
// Layout.  Everything is computed TRANSPOSED, as enc_attn.hip's fused kernels do, so that a tile of scores never changes layout
// between the product that forms it and the product that reads it.  In the 32x32 C layout lane n = lane & 31 is a column and the 16
// registers are rows (r & 3) + 8 (r >> 2) + 4 (lane >> 5); registers 8 g .. 8 g + 7 go straight back in as the B operand of a k step
// whose eight k of lane half lk are rows 16 s + {4 lk .. + 3} and 16 s + 8 + {4 lk .. + 3}, and the A operand is read from a
// TRANSPOSED LDS image [dim][row of the tile] by the same map (frag_tr).
//   forward, dQ:  S^T = K Q^T, the lane is a QUERY (its Q / dctx rows and statistics stay in registers), registers are keys;
//                 O^T += V^T P^T, dQ^T += K^T dS^T
//   dK, dV:       S = Q K^T, the lane is a KEY (its K / V rows stay in registers), registers are queries (their statistics come from
//                 LDS); dV^T += dctx^T P_drop, dK^T += Q^T dS
// A wave owns 32 lanes' rows, a workgroup 128; the other side is walked in tiles of 64 rows staged in LDS as bf16, 144-byte rows (64
// values + 16 bytes: the 16-byte fragment reads of consecutive rows fall 36 banks apart).
//
// Masks (the rules above flash_attn_f32_kernel, enc_attn.hip): a masked key adds the finite -FLT_MAX, a tile-padding key (beyond L)
// -inf, which a tile never holds alone (tiles start below L); a row without a real key attends uniformly over its L keys, which is
// why m and l are kept apart: -FLT_MAX + log2(L) rounds back to -FLT_MAX.  In the backward, query rows and key rows beyond L contribute
// exact zeros by a SELECT on P_drop and dS (their statistics are never read, their staged operand rows are zeros).
//
// Dropout (dropout_rng.h): site 1 + 3 l on the logical index ((b H + h) L + i) L + j.  Where the lane is a query its four consecutive
// keys share one Philox block when L % 4 == 0 (one draw per four elements); otherwise, and wherever the lane is a key, every element
// is keyed on its own index.  DROP = false instantiations contain no generator.
//
// Packed rows (the padding-free mode; the PackedDocs instantiations of the four kernels, the _packed launchers and debug entries): the
// row tensors hold the valid tokens alone, document b's at rows doc_start[b] .. doc_start[b + 1] - 1.  A workgroup's (document, head,
// block) comes from the grid as above, sized by the LONGEST document; it reads its document's start and length and leaves at once
// when its block starts at or beyond the length -- uniform per workgroup, before the first barrier.  Every key of a document is real,
// so the only bias is -inf on tile padding beyond the length and no mask is read; statistics are [H, rows, 2] and D [H, rows], by
// packed row.  Dropout keys are the PADDED call's: the positions i, j of ((b H + h) Lpad + i) Lpad + j come from row_src (the keys'
// through LDS, the queries' of the key-block kernel as whole 64-bit keys through LDS), so a packed step draws the padded step's masks;
// one draw per four keys only when every document is a prefix and Lpad % 4 == 0.  The padded instantiations are compiled from the
// same text with every packed branch an `if constexpr`: same instruction counts, registers and LDS as before the second layout.
#include <math.h>

#include "enc_host.h"
#include "enc_stage.h"

namespace aspire {
namespace {

constexpr int kTLd = 72;                                             // bf16 per LDS row
constexpr float kTScaleLog2 = 0.125f * 1.44269504088896340736f;      // 1 / sqrt(64) folded with log2(e)
typedef uint16_t TrainTile[64][kTLd];

__device__ __forceinline__ float train_key_bias(const int64_t* __restrict__ mask_row, int kk, int L) {
    return kk >= L ? -INFINITY : (mask_row[kk] != 0 ? 0.f : -3.4028234663852886e38f);
}

// rows r0 .. r0 + 63 of src (64 columns, row stride ld) -> T [row][dim]; rows beyond L are zeros (nothing is read past row L - 1)
__device__ __forceinline__ void stage_rows(TrainTile& T, const float* __restrict__ src, size_t ld, int r0, int L, int tid) {
    const int row = tid >> 2, d0 = (tid & 3) * 16;
    const bool ok = r0 + row < L;
    const float* p = src + (size_t)min(r0 + row, L - 1) * ld + d0;
    uint32_t w[8];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        float4 v = *reinterpret_cast<const float4*>(p + 4 * c);
        if (!ok) v = make_float4(0.f, 0.f, 0.f, 0.f);
        w[2 * c] = pack_bf16(v.x, v.y);
        w[2 * c + 1] = pack_bf16(v.z, v.w);
    }
    *reinterpret_cast<uint4*>(&T[row][d0]) = make_uint4(w[0], w[1], w[2], w[3]);
    *reinterpret_cast<uint4*>(&T[row][d0 + 8]) = make_uint4(w[4], w[5], w[6], w[7]);
}

// the same rows -> T [dim][row of the tile]: a thread turns 4 rows x 4 dims in registers and writes 8-byte runs of four rows
__device__ __forceinline__ void stage_cols(TrainTile& T, const float* __restrict__ src, size_t ld, int r0, int L, int tid) {
    const int rg = tid >> 4, dg = tid & 15;
    float4 v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int row = r0 + 4 * rg + k;
        v[k] = *reinterpret_cast<const float4*>(src + (size_t)min(row, L - 1) * ld + 4 * dg);
        if (row >= L) v[k] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    *reinterpret_cast<uint2*>(&T[4 * dg + 0][4 * rg]) = make_uint2(pack_bf16(v[0].x, v[1].x), pack_bf16(v[2].x, v[3].x));
    *reinterpret_cast<uint2*>(&T[4 * dg + 1][4 * rg]) = make_uint2(pack_bf16(v[0].y, v[1].y), pack_bf16(v[2].y, v[3].y));
    *reinterpret_cast<uint2*>(&T[4 * dg + 2][4 * rg]) = make_uint2(pack_bf16(v[0].z, v[1].z), pack_bf16(v[2].z, v[3].z));
    *reinterpret_cast<uint2*>(&T[4 * dg + 3][4 * rg]) = make_uint2(pack_bf16(v[0].w, v[1].w), pack_bf16(v[2].w, v[3].w));
}

// fragment of a [row][dim] image: dims 16 ks + 8 lk .. + 7 of one row
__device__ __forceinline__ bf16x8_t frag_rm(const TrainTile& T, int row, int ks, int lk) {
    return __builtin_bit_cast(bf16x8_t, *reinterpret_cast<const uint4*>(&T[row][16 * ks + 8 * lk]));
}
// fragment of a [dim][row] image: rows 16 s + {4 lk .. + 3} and 16 s + 8 + {4 lk .. + 3} of one dim (the rows that registers
// 8 g .. 8 g + 7 of a C tile hold in lane half lk)
__device__ __forceinline__ bf16x8_t frag_tr(const TrainTile& T, int dim, int s, int lk) {
    const uint2 lo = *reinterpret_cast<const uint2*>(&T[dim][16 * s + 4 * lk]);
    const uint2 hi = *reinterpret_cast<const uint2*>(&T[dim][16 * s + 8 + 4 * lk]);
    return __builtin_bit_cast(bf16x8_t, make_uint4(lo.x, lo.y, hi.x, hi.y));
}
// this lane's row of a [rows, ld] fp32 tensor as the four B fragments of a product over the 64 dims
__device__ __forceinline__ void row_frags(const float* __restrict__ p, int lk, bf16x8_t (&f)[4]) {
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
        const float4 u = *reinterpret_cast<const float4*>(p + 16 * ks + 8 * lk), v = *reinterpret_cast<const float4*>(p + 16 * ks + 8 * lk + 4);
        f[ks] = __builtin_bit_cast(bf16x8_t, make_uint4(pack_bf16(u.x, u.y), pack_bf16(u.z, u.w), pack_bf16(v.x, v.y), pack_bf16(v.z, v.w)));
    }
}
__device__ __forceinline__ bf16x8_t pack8(const float (&x)[8]) {
    return __builtin_bit_cast(bf16x8_t, make_uint4(pack_bf16(x[0], x[1]), pack_bf16(x[2], x[3]), pack_bf16(x[4], x[5]), pack_bf16(x[6], x[7])));
}
__device__ __forceinline__ f32x16 zero16() {
    f32x16 z;
#pragma unroll
    for (int r = 0; r < 16; ++r) z[r] = 0.f;
    return z;
}

// keep . scale of elements e0 .. e0 + 3 (consecutive keys of one query); aligned: e0 % 4 == 0, one Philox block
__device__ __forceinline__ void keep_scale4(const DropSite& d, uint64_t e0, bool aligned, float (&f)[4]) {
    if (aligned) {
        const Philox4 r = drop_block(d, e0 >> 2);
#pragma unroll
        for (int i = 0; i < 4; ++i) f[i] = r.w[i] >= d.thr ? d.scale : 0.f;
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) f[i] = drop_keep(d, e0 + i) ? d.scale : 0.f;
    }
}

// the same over packed rows: keys key0 .. key0 + 3 of the tile at k0 sit at positions kpos[key0 ..] of the padded document.  quad (every
// document a prefix, Lpad % 4 == 0): their positions are k0 + key0 .. + 3 and start a Philox block; otherwise every element is keyed on
// its own index.  The mask bits are the same either way.
__device__ __forceinline__ void keep_scale4_at(const DropSite& d, uint64_t e_row, int k0, const int* kpos, int key0, bool quad, float (&f)[4]) {
    if (quad) {
        const Philox4 r = drop_block(d, (e_row + (uint64_t)(k0 + key0)) >> 2);
#pragma unroll
        for (int i = 0; i < 4; ++i) f[i] = r.w[i] >= d.thr ? d.scale : 0.f;
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) f[i] = drop_keep(d, e_row + (uint64_t)kpos[key0 + i]) ? d.scale : 0.f;
    }
}

// (document, head, block) of a workgroup
__device__ __forceinline__ void block_ids(int blocks, int H, int& blk, int& h, int& b) {
    blk = blockIdx.x % blocks;
    h = (blockIdx.x / blocks) % H;
    b = blockIdx.x / (blocks * H);
}

// Where a document's rows lie.  PaddedDocs: document b's L rows at b L of [B L, .] tensors, statistics [B, H, L], the caller's mask.
// PackedDocs (enc_types.h): its len = doc_start[b + 1] - doc_start[b] rows at doc_start[b] of [rows, .] tensors, statistics [H, rows],
// no mask (every key is real); L is then the longest document, which sizes the grid alone.  The padded instantiations are the code
// they were before there was a second layout: every packed branch is an `if constexpr`.
struct PaddedDocs {
    const int64_t* mask;
};
template <class Docs>
constexpr bool kPackedDocs = false;
template <>
constexpr bool kPackedDocs<PackedDocs> = true;

struct DocRows {
    int len;          // rows of the document
    size_t row0;      // its first row in qkv / ctx / dctx / dqkv
    size_t stat0;     // the index of that row's statistics (and D) for head h
    int pos0;         // packed: b Lpad, what row_src counts a position from
};
__device__ __forceinline__ DocRows doc_rows(const PaddedDocs&, int b, int h, int L, int H) {
    return DocRows{L, (size_t)b * L, ((size_t)b * H + h) * L, 0};
}
// (clamped, so that no content of doc_start takes a row index outside [0, rows] or a length beyond L)
__device__ __forceinline__ DocRows doc_rows(const PackedDocs& d, int b, int h, int L, int) {
    const int start = min(max(d.doc_start[b], 0), d.rows), end = min(max(d.doc_start[b + 1], start), d.rows);
    return DocRows{min(end - start, L), (size_t)start, (size_t)h * d.rows + start, b * d.Lpad};
}
// the dropout key of element (query at position pi, key 0) of (document b, head h) in the PADDED tensor [B, H, Lpad, Lpad]
__device__ __forceinline__ uint64_t packed_e_row(const PackedDocs& d, int b, int h, int H, int pi) {
    return ((uint64_t)(b * H + h) * d.Lpad + (uint64_t)pi) * d.Lpad;
}

template <bool DROP, class Docs>
__global__ void __launch_bounds__(256) flash_train_fwd_kernel(const float* __restrict__ qkv, const Docs docs,
                                                              float* __restrict__ ctx, float* __restrict__ stats, int L, int H, DropSite ds) {
    constexpr bool PACKED = kPackedDocs<Docs>;
    __shared__ __attribute__((aligned(16))) TrainTile Ks, Vt;          // K [key][dim], V [dim][key]
    __shared__ float kbias[64];
    __shared__ int kpos[PACKED ? 64 : 1];                              // packed: the keys' positions in their padded document
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lr = lane & 31, lk = lane >> 5;
    int qb, h, b;
    block_ids((L + 127) / 128, H, qb, h, b);
    const DocRows doc = doc_rows(docs, b, h, L, H);
    if constexpr (PACKED) {
        if (qb * 128 >= doc.len) return;                               // uniform per workgroup, before the first barrier
        L = doc.len;
    }
    const size_t ld = 3 * kD;
    const float* base = qkv + doc.row0 * ld + h * 64;
    const int q_row = qb * 128 + wave * 32 + lr;                      // this lane's query
    const bool q_ok = q_row < L;
    bf16x8_t qf[4];
    row_frags(base + (size_t)min(q_row, L - 1) * ld, lk, qf);
    f32x16 o[2] = {zero16(), zero16()};
    float m_run = -INFINITY, l_run = 0.f;                              // l_run: this half-wave's share of the sum
    uint64_t e_row;
    bool aligned;
    if constexpr (PACKED) {
        e_row = packed_e_row(docs, b, h, H, docs.row_src[doc.row0 + min(q_row, L - 1)] - doc.pos0);
        aligned = docs.quad != 0;
    } else {
        e_row = ((uint64_t)(b * H + h) * L + (uint64_t)min(q_row, L - 1)) * L;
        aligned = (L & 3) == 0;
    }

    for (int k0 = 0; k0 < L; k0 += 64) {
        __syncthreads();                                               // previous tile fully consumed
        stage_rows(Ks, base + kD, ld, k0, L, tid);
        stage_cols(Vt, base + 2 * kD, ld, k0, L, tid);
        if constexpr (PACKED) {
            if (tid < 64) {
                kbias[tid] = k0 + tid >= L ? -INFINITY : 0.f;
                kpos[tid] = docs.row_src[doc.row0 + min(k0 + tid, L - 1)] - doc.pos0;
            }
        } else {
            if (tid < 64) kbias[tid] = train_key_bias(docs.mask + (size_t)b * L, k0 + tid, L);
        }
        __syncthreads();
        f32x16 sacc[2] = {zero16(), zero16()};
#pragma unroll
        for (int ks = 0; ks < 4; ++ks)
#pragma unroll
            for (int rb = 0; rb < 2; ++rb) sacc[rb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_rm(Ks, 32 * rb + lr, ks, lk), qf[ks], sacc[rb], 0, 0, 0);
        float tmax = -INFINITY;
#pragma unroll
        for (int rb = 0; rb < 2; ++rb)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int key = 32 * rb + 8 * (r >> 2) + 4 * lk + (r & 3);
                sacc[rb][r] = fmaf(sacc[rb][r], kTScaleLog2, kbias[key]);
                tmax = fmaxf(tmax, sacc[rb][r]);
            }
        tmax = fmaxf(tmax, lane_xor<32>(tmax));
        const float m_new = fmaxf(m_run, tmax);
        const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);     // exp2(-inf) = 0 on the first tile
        float psum = 0.f;
#pragma unroll
        for (int rb = 0; rb < 2; ++rb)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                sacc[rb][r] = __builtin_amdgcn_exp2f(sacc[rb][r] - m_new);
                psum += sacc[rb][r];                                   // the sum is of the undropped probabilities
            }
        l_run = fmaf(l_run, alpha, psum);
        m_run = m_new;
#pragma unroll
        for (int mb = 0; mb < 2; ++mb)
#pragma unroll
            for (int r = 0; r < 16; ++r) o[mb][r] *= alpha;
#pragma unroll
        for (int rb = 0; rb < 2; ++rb)
#pragma unroll
            for (int g2 = 0; g2 < 2; ++g2) {
                float pv[8];
#pragma unroll
                for (int e = 0; e < 8; ++e) pv[e] = sacc[rb][8 * g2 + e];
                if constexpr (DROP) {
#pragma unroll
                    for (int q4 = 0; q4 < 2; ++q4) {
                        float f[4];
                        if constexpr (PACKED)
                            keep_scale4_at(ds, e_row, k0, kpos, 32 * rb + 16 * g2 + 8 * q4 + 4 * lk, aligned, f);
                        else
                            keep_scale4(ds, e_row + (uint64_t)(k0 + 32 * rb + 16 * g2 + 8 * q4 + 4 * lk), aligned, f);
#pragma unroll
                        for (int i = 0; i < 4; ++i) pv[4 * q4 + i] *= f[i];
                    }
                }
                const bf16x8_t pb = pack8(pv);
#pragma unroll
                for (int mb = 0; mb < 2; ++mb)
                    o[mb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_tr(Vt, 32 * mb + lr, 2 * rb + g2, lk), pb, o[mb], 0, 0, 0);
            }
    }
    const float l_tot = l_run + lane_xor<32>(l_run);
    const float inv = 1.0f / l_tot;
    if (q_ok) {
        float* op = ctx + (doc.row0 + q_row) * kD + h * 64;
#pragma unroll
        for (int mb = 0; mb < 2; ++mb)
#pragma unroll
            for (int g4 = 0; g4 < 4; ++g4)
                *reinterpret_cast<float4*>(op + 32 * mb + 8 * g4 + 4 * lk) =
                    make_float4(o[mb][4 * g4 + 0] * inv, o[mb][4 * g4 + 1] * inv, o[mb][4 * g4 + 2] * inv, o[mb][4 * g4 + 3] * inv);
        if (lk == 0) *reinterpret_cast<float2*>(stats + 2 * (doc.stat0 + q_row)) = make_float2(m_run, l_tot);
    }
}

// 16 lanes per (token row, head).  PACKED: D [H, L] with L the packed rows, the row tensors' rows as they are
template <bool PACKED>
__global__ void __launch_bounds__(256) flash_train_d_kernel(const float* __restrict__ dctx, const float* __restrict__ ctx, float* __restrict__ D,
                                                            int64_t items, int L, int H) {
    const int64_t item = (int64_t)blockIdx.x * 16 + (threadIdx.x >> 4);
    const int l16 = threadIdx.x & 15;
    const int64_t it = item < items ? item : items - 1;
    const int64_t row = it / H;
    const int h = (int)(it % H);
    const size_t at = (size_t)row * kD + h * 64 + 4 * l16;
    // dctx as the products with it see it, rounded to bf16: D stands for rowsum(dP . P) with dP = bf16(dctx) bf16(V)^T, and the rows of
    // dS = P (dP - D) sum to zero only as far as the two agree (the key bias's gradient, zero in exact arithmetic, is that sum)
    const float4 g = *reinterpret_cast<const float4*>(dctx + at), c = *reinterpret_cast<const float4*>(ctx + at);
    const uint32_t xy = pack_bf16(g.x, g.y), zw = pack_bf16(g.z, g.w);
    const float4 a = make_float4(__builtin_bit_cast(float, xy << 16), __builtin_bit_cast(float, xy & 0xffff0000u),
                                 __builtin_bit_cast(float, zw << 16), __builtin_bit_cast(float, zw & 0xffff0000u));
    float s = fmaf(a.w, c.w, fmaf(a.z, c.z, fmaf(a.y, c.y, a.x * c.x)));
    s += __shfl_xor(s, 8, 16);
    s += __shfl_xor(s, 4, 16);
    s += __shfl_xor(s, 2, 16);
    s += __shfl_xor(s, 1, 16);
    if constexpr (PACKED) {
        if (l16 == 0 && item < items) D[(int64_t)h * L + row] = s;
    } else {
        if (l16 == 0 && item < items) D[((row / L) * H + h) * L + row % L] = s;
    }
}

template <bool DROP, class Docs>
__global__ void __launch_bounds__(256) flash_train_dq_kernel(const float* __restrict__ qkv, const Docs docs,
                                                             const float* __restrict__ stats, const float* __restrict__ Dv,
                                                             const float* __restrict__ dctx, float* __restrict__ dqkv, int L, int H, DropSite ds) {
    constexpr bool PACKED = kPackedDocs<Docs>;
    __shared__ __attribute__((aligned(16))) TrainTile Ks, Vs, Kt;      // K [key][dim], V [key][dim], K [dim][key]
    __shared__ float kbias[64];
    __shared__ int kpos[PACKED ? 64 : 1];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lr = lane & 31, lk = lane >> 5;
    int qb, h, b;
    block_ids((L + 127) / 128, H, qb, h, b);
    const DocRows doc = doc_rows(docs, b, h, L, H);
    if constexpr (PACKED) {
        if (qb * 128 >= doc.len) return;
        L = doc.len;
    }
    const size_t ld = 3 * kD;
    const float* base = qkv + doc.row0 * ld + h * 64;
    const int q_row = qb * 128 + wave * 32 + lr;                      // this lane's query
    const bool q_ok = q_row < L;
    const int q_at = min(q_row, L - 1);
    bf16x8_t qf[4], gf[4];
    row_frags(base + (size_t)q_at * ld, lk, qf);
    row_frags(dctx + (doc.row0 + q_at) * kD + h * 64, lk, gf);
    const size_t s_at = doc.stat0 + q_at;
    const float m = stats[2 * s_at], linv = 1.0f / stats[2 * s_at + 1], Dq = Dv[s_at];
    uint64_t e_row;
    bool aligned;
    if constexpr (PACKED) {
        e_row = packed_e_row(docs, b, h, H, docs.row_src[doc.row0 + q_at] - doc.pos0);
        aligned = docs.quad != 0;
    } else {
        e_row = (uint64_t)s_at * L;
        aligned = (L & 3) == 0;
    }
    f32x16 dq[2] = {zero16(), zero16()};

    for (int k0 = 0; k0 < L; k0 += 64) {
        __syncthreads();
        stage_rows(Ks, base + kD, ld, k0, L, tid);
        stage_rows(Vs, base + 2 * kD, ld, k0, L, tid);
        stage_cols(Kt, base + kD, ld, k0, L, tid);
        if constexpr (PACKED) {
            if (tid < 64) {
                kbias[tid] = k0 + tid >= L ? -INFINITY : 0.f;
                kpos[tid] = docs.row_src[doc.row0 + min(k0 + tid, L - 1)] - doc.pos0;
            }
        } else {
            if (tid < 64) kbias[tid] = train_key_bias(docs.mask + (size_t)b * L, k0 + tid, L);
        }
        __syncthreads();
        f32x16 s[2] = {zero16(), zero16()}, dp[2] = {zero16(), zero16()};
#pragma unroll
        for (int ks = 0; ks < 4; ++ks)
#pragma unroll
            for (int rb = 0; rb < 2; ++rb) {
                s[rb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_rm(Ks, 32 * rb + lr, ks, lk), qf[ks], s[rb], 0, 0, 0);
                dp[rb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_rm(Vs, 32 * rb + lr, ks, lk), gf[ks], dp[rb], 0, 0, 0);
            }
#pragma unroll
        for (int rb = 0; rb < 2; ++rb)
#pragma unroll
            for (int g2 = 0; g2 < 2; ++g2) {
                float dsv[8];
#pragma unroll
                for (int q4 = 0; q4 < 2; ++q4) {
                    const int key0 = 32 * rb + 16 * g2 + 8 * q4 + 4 * lk;
                    float f[4] = {1.f, 1.f, 1.f, 1.f};
                    if constexpr (DROP) {
                        if constexpr (PACKED)
                            keep_scale4_at(ds, e_row, k0, kpos, key0, aligned, f);
                        else
                            keep_scale4(ds, e_row + (uint64_t)(k0 + key0), aligned, f);
                    }
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const int r = 8 * g2 + 4 * q4 + i;
                        const float p = __builtin_amdgcn_exp2f(fmaf(s[rb][r], kTScaleLog2, kbias[key0 + i]) - m) * linv;
                        const float g = DROP ? dp[rb][r] * f[i] : dp[rb][r];
                        dsv[4 * q4 + i] = (q_ok && k0 + key0 + i < L) ? p * (g - Dq) : 0.f;
                    }
                }
                const bf16x8_t db = pack8(dsv);
#pragma unroll
                for (int mb = 0; mb < 2; ++mb)
                    dq[mb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_tr(Kt, 32 * mb + lr, 2 * rb + g2, lk), db, dq[mb], 0, 0, 0);
            }
    }
    if (q_ok) {
        float* op = dqkv + (doc.row0 + q_row) * ld + h * 64;
#pragma unroll
        for (int mb = 0; mb < 2; ++mb)
#pragma unroll
            for (int g4 = 0; g4 < 4; ++g4)
                *reinterpret_cast<float4*>(op + 32 * mb + 8 * g4 + 4 * lk) = make_float4(dq[mb][4 * g4 + 0] * 0.125f, dq[mb][4 * g4 + 1] * 0.125f,
                                                                                        dq[mb][4 * g4 + 2] * 0.125f, dq[mb][4 * g4 + 3] * 0.125f);
    }
}

template <bool DROP, class Docs>
__global__ void __launch_bounds__(256) flash_train_dkv_kernel(const float* __restrict__ qkv, const Docs docs,
                                                              const float* __restrict__ stats, const float* __restrict__ Dv,
                                                              const float* __restrict__ dctx, float* __restrict__ dqkv, int L, int H, DropSite ds) {
    constexpr bool PACKED = kPackedDocs<Docs>;
    __shared__ __attribute__((aligned(16))) TrainTile Qs, Gs, Qt, Gt;  // Q, dctx [query][dim]; Q, dctx [dim][query]
    __shared__ float st_m[64], st_linv[64], st_d[64];
    __shared__ unsigned long long st_e[PACKED && DROP ? 64 : 1];      // packed: the queries' dropout keys at key position 0
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lr = lane & 31, lk = lane >> 5;
    int kb, h, b;
    block_ids((L + 127) / 128, H, kb, h, b);
    const DocRows doc = doc_rows(docs, b, h, L, H);
    if constexpr (PACKED) {
        if (kb * 128 >= doc.len) return;
        L = doc.len;
    }
    const size_t ld = 3 * kD;
    const float* base = qkv + doc.row0 * ld + h * 64;
    const float* gbase = dctx + doc.row0 * kD + h * 64;
    const int k_row = kb * 128 + wave * 32 + lr;                      // this lane's key
    const bool k_ok = k_row < L;
    const int k_at = min(k_row, L - 1);
    bf16x8_t kf[4], vf[4];
    row_frags(base + kD + (size_t)k_at * ld, lk, kf);
    row_frags(base + 2 * kD + (size_t)k_at * ld, lk, vf);
    float kbias;
    [[maybe_unused]] uint64_t k_pos = 0;                               // packed: this lane's key's position in its padded document
    if constexpr (PACKED) {
        kbias = k_row >= L ? -INFINITY : 0.f;
        if constexpr (DROP) k_pos = (uint64_t)(docs.row_src[doc.row0 + k_at] - doc.pos0);
    } else {
        kbias = train_key_bias(docs.mask + (size_t)b * L, k_row, L);
    }
    const size_t s_doc = doc.stat0;
    f32x16 dv[2] = {zero16(), zero16()}, dk[2] = {zero16(), zero16()};

    for (int q0 = 0; q0 < L; q0 += 64) {
        __syncthreads();
        stage_rows(Qs, base, ld, q0, L, tid);
        stage_rows(Gs, gbase, kD, q0, L, tid);
        stage_cols(Qt, base, ld, q0, L, tid);
        stage_cols(Gt, gbase, kD, q0, L, tid);
        if (tid < 64) {
            const bool ok = q0 + tid < L;
            const size_t at = s_doc + min(q0 + tid, L - 1);
            st_m[tid] = ok ? stats[2 * at] : 0.f;
            st_linv[tid] = ok ? 1.0f / stats[2 * at + 1] : 0.f;
            st_d[tid] = ok ? Dv[at] : 0.f;
            if constexpr (PACKED && DROP)
                st_e[tid] = packed_e_row(docs, b, h, H, docs.row_src[doc.row0 + min(q0 + tid, L - 1)] - doc.pos0);
        }
        __syncthreads();
        f32x16 s[2] = {zero16(), zero16()}, dp[2] = {zero16(), zero16()};
#pragma unroll
        for (int ks = 0; ks < 4; ++ks)
#pragma unroll
            for (int rb = 0; rb < 2; ++rb) {
                s[rb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_rm(Qs, 32 * rb + lr, ks, lk), kf[ks], s[rb], 0, 0, 0);
                dp[rb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_rm(Gs, 32 * rb + lr, ks, lk), vf[ks], dp[rb], 0, 0, 0);
            }
#pragma unroll
        for (int rb = 0; rb < 2; ++rb)
#pragma unroll
            for (int g2 = 0; g2 < 2; ++g2) {
                float pd[8], dsv[8];
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const int r = 8 * g2 + e, qi = 32 * rb + 16 * g2 + 8 * (e >> 2) + 4 * lk + (e & 3);
                    const bool ok = k_ok && q0 + qi < L;
                    const float p = __builtin_amdgcn_exp2f(fmaf(s[rb][r], kTScaleLog2, kbias) - st_m[qi]) * st_linv[qi];
                    float f = 1.f;
                    if constexpr (DROP) {
                        if constexpr (PACKED)
                            f = drop_keep(ds, st_e[qi] + k_pos) ? ds.scale : 0.f;
                        else
                            f = drop_keep(ds, (uint64_t)(s_doc + min(q0 + qi, L - 1)) * L + (uint64_t)k_at) ? ds.scale : 0.f;
                    }
                    const float g = DROP ? dp[rb][r] * f : dp[rb][r];
                    pd[e] = ok ? (DROP ? p * f : p) : 0.f;
                    dsv[e] = ok ? p * (g - st_d[qi]) : 0.f;
                }
                const bf16x8_t pb = pack8(pd), db = pack8(dsv);
#pragma unroll
                for (int mb = 0; mb < 2; ++mb) {
                    dv[mb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_tr(Gt, 32 * mb + lr, 2 * rb + g2, lk), pb, dv[mb], 0, 0, 0);
                    dk[mb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_tr(Qt, 32 * mb + lr, 2 * rb + g2, lk), db, dk[mb], 0, 0, 0);
                }
            }
    }
    if (k_ok) {
        float* op = dqkv + (doc.row0 + k_row) * ld + kD + h * 64;
#pragma unroll
        for (int mb = 0; mb < 2; ++mb)
#pragma unroll
            for (int g4 = 0; g4 < 4; ++g4) {
                *reinterpret_cast<float4*>(op + 32 * mb + 8 * g4 + 4 * lk) = make_float4(dk[mb][4 * g4 + 0] * 0.125f, dk[mb][4 * g4 + 1] * 0.125f,
                                                                                        dk[mb][4 * g4 + 2] * 0.125f, dk[mb][4 * g4 + 3] * 0.125f);
                *reinterpret_cast<float4*>(op + kD + 32 * mb + 8 * g4 + 4 * lk) =
                    make_float4(dv[mb][4 * g4 + 0], dv[mb][4 * g4 + 1], dv[mb][4 * g4 + 2], dv[mb][4 * g4 + 3]);
            }
    }
}

int check_flash_shape(int64_t B, int64_t L, int H) {
    ASPIRE_REQUIRE(B >= 0 && L > 0 && L <= 512, ASPIRE_ERR_INVALID_ARG, "sequence length %lld outside (0, 512] (or a negative batch size)",
                   (long long)L);
    ASPIRE_REQUIRE(H == 12, ASPIRE_ERR_UNSUPPORTED, "the fused training attention is built for 12 heads of 64; got %d heads", H);
    ASPIRE_REQUIRE((double)B * H * ((L + 127) / 128) < 2147483648.0 && (double)B * L * 3 * kD < 2147483648.0, ASPIRE_ERR_UNSUPPORTED,
                   "%lld documents of %lld tokens in one call: beyond the grid (split the batch)", (long long)B, (long long)L);
    return ASPIRE_OK;
}

}  // namespace

int launch_flash_attn_train(const float* qkv, const int64_t* mask, float* ctx, float* stats, int64_t B, int L, int H, const DropSite* drop,
                            hipStream_t st) {
    if (int rc = check_flash_shape(B, L, H)) return rc;
    if (B == 0) return ASPIRE_OK;
    const dim3 grid((unsigned)(B * H) * (unsigned)((L + 127) / 128));
    const PaddedDocs docs{mask};
    if (drop)
        hipLaunchKernelGGL((flash_train_fwd_kernel<true, PaddedDocs>), grid, dim3(256), 0, st, qkv, docs, ctx, stats, L, H, *drop);
    else
        hipLaunchKernelGGL((flash_train_fwd_kernel<false, PaddedDocs>), grid, dim3(256), 0, st, qkv, docs, ctx, stats, L, H, DropSite{});
    ASPIRE_LAUNCH_OK();
    return ASPIRE_OK;
}

namespace {
// the packed calls' shape: the grid is sized by the longest document, the row tensors by the packed rows
int check_flash_packed(int64_t B, const PackedDocs& d, int max_len, int H) {
    ASPIRE_REQUIRE(d.doc_start && d.row_src, ASPIRE_ERR_INVALID_ARG, "null pointer (doc_start / row_src)");
    ASPIRE_REQUIRE(d.rows > 0 && max_len > 0 && max_len <= d.Lpad && max_len <= d.rows, ASPIRE_ERR_INVALID_ARG,
                   "packing: %d rows, longest document %d of %d padded tokens", d.rows, max_len, d.Lpad);
    if (int rc = check_flash_shape(B, d.Lpad, H)) return rc;
    ASPIRE_REQUIRE((double)d.rows * 3 * kD < 2147483648.0, ASPIRE_ERR_UNSUPPORTED, "%d packed rows in one call: beyond the grid (split the batch)",
                   d.rows);
    return ASPIRE_OK;
}
}  // namespace

int launch_flash_attn_train_packed(const float* qkv, const PackedDocs& docs, int max_len, float* ctx, float* stats, int64_t B, int H,
                                   const DropSite* drop, hipStream_t st) {
    if (B == 0 || docs.rows == 0) return ASPIRE_OK;
    if (int rc = check_flash_packed(B, docs, max_len, H)) return rc;
    const dim3 grid((unsigned)(B * H) * (unsigned)((max_len + 127) / 128));
    if (drop)
        hipLaunchKernelGGL((flash_train_fwd_kernel<true, PackedDocs>), grid, dim3(256), 0, st, qkv, docs, ctx, stats, max_len, H, *drop);
    else
        hipLaunchKernelGGL((flash_train_fwd_kernel<false, PackedDocs>), grid, dim3(256), 0, st, qkv, docs, ctx, stats, max_len, H, DropSite{});
    ASPIRE_LAUNCH_OK();
    return ASPIRE_OK;
}

int launch_flash_attn_train_backward_packed(const float* qkv, const PackedDocs& docs, int max_len, const float* ctx, const float* stats,
                                            const float* dctx, float* D, float* dqkv, int64_t B, int H, const DropSite* drop, hipStream_t st) {
    if (B == 0 || docs.rows == 0) return ASPIRE_OK;
    if (int rc = check_flash_packed(B, docs, max_len, H)) return rc;
    const int64_t items = (int64_t)docs.rows * H;
    hipLaunchKernelGGL(flash_train_d_kernel<true>, dim3((unsigned)((items + 15) / 16)), dim3(256), 0, st, dctx, ctx, D, items, docs.rows, H);
    ASPIRE_LAUNCH_OK();
    const dim3 grid((unsigned)(B * H) * (unsigned)((max_len + 127) / 128));
    if (drop) {
        hipLaunchKernelGGL((flash_train_dkv_kernel<true, PackedDocs>), grid, dim3(256), 0, st, qkv, docs, stats, D, dctx, dqkv, max_len, H, *drop);
        ASPIRE_LAUNCH_OK();
        hipLaunchKernelGGL((flash_train_dq_kernel<true, PackedDocs>), grid, dim3(256), 0, st, qkv, docs, stats, D, dctx, dqkv, max_len, H, *drop);
    } else {
        hipLaunchKernelGGL((flash_train_dkv_kernel<false, PackedDocs>), grid, dim3(256), 0, st, qkv, docs, stats, D, dctx, dqkv, max_len, H,
                           DropSite{});
        ASPIRE_LAUNCH_OK();
        hipLaunchKernelGGL((flash_train_dq_kernel<false, PackedDocs>), grid, dim3(256), 0, st, qkv, docs, stats, D, dctx, dqkv, max_len, H,
                           DropSite{});
    }
    ASPIRE_LAUNCH_OK();
    return ASPIRE_OK;
}

int launch_flash_attn_train_backward(const float* qkv, const int64_t* mask, const float* ctx, const float* stats, const float* dctx, float* D,
                                     float* dqkv, int64_t B, int L, int H, const DropSite* drop, hipStream_t st) {
    if (int rc = check_flash_shape(B, L, H)) return rc;
    if (B == 0) return ASPIRE_OK;
    const int64_t items = B * L * H;
    hipLaunchKernelGGL(flash_train_d_kernel<false>, dim3((unsigned)((items + 15) / 16)), dim3(256), 0, st, dctx, ctx, D, items, L, H);
    ASPIRE_LAUNCH_OK();
    const dim3 grid((unsigned)(B * H) * (unsigned)((L + 127) / 128));
    const PaddedDocs docs{mask};
    if (drop) {
        hipLaunchKernelGGL((flash_train_dkv_kernel<true, PaddedDocs>), grid, dim3(256), 0, st, qkv, docs, stats, D, dctx, dqkv, L, H, *drop);
        ASPIRE_LAUNCH_OK();
        hipLaunchKernelGGL((flash_train_dq_kernel<true, PaddedDocs>), grid, dim3(256), 0, st, qkv, docs, stats, D, dctx, dqkv, L, H, *drop);
    } else {
        hipLaunchKernelGGL((flash_train_dkv_kernel<false, PaddedDocs>), grid, dim3(256), 0, st, qkv, docs, stats, D, dctx, dqkv, L, H, DropSite{});
        ASPIRE_LAUNCH_OK();
        hipLaunchKernelGGL((flash_train_dq_kernel<false, PaddedDocs>), grid, dim3(256), 0, st, qkv, docs, stats, D, dctx, dqkv, L, H, DropSite{});
    }
    ASPIRE_LAUNCH_OK();
    return ASPIRE_OK;
}

}  // namespace aspire

using namespace aspire;

namespace {
// the attention site of `layer` from the caller's struct; *on = false: no dropout there (NULL, or p_attn == 0)
int debug_site(const aspire_bert_dropout* d, int layer, DropSite* site, bool* on) {
    *on = false;
    if (!d) return ASPIRE_OK;
    ASPIRE_REQUIRE(d->p_attn >= 0.f && d->p_attn < 1.f, ASPIRE_ERR_INVALID_ARG, "dropout probability p_attn = %g outside [0, 1)", (double)d->p_attn);
    ASPIRE_REQUIRE(layer >= 0 && layer < (1 << 20), ASPIRE_ERR_INVALID_ARG, "layer %d", layer);
    if (d->p_attn > 0.f) {
        *site = drop_site(d->seed, d->step, 1 + 3 * (uint32_t)layer, d->p_attn);
        *on = true;
    }
    return ASPIRE_OK;
}
}  // namespace

extern "C" int aspire_debug_flash_attn_train_f32(const float* qkv, const int64_t* mask, int64_t B, int64_t L, const aspire_bert_dropout* dropout,
                                                 float* ctx, float* stats, void* stream) {
    ASPIRE_REQUIRE(qkv && mask && ctx && stats, ASPIRE_ERR_INVALID_ARG, "null pointer");
    DropSite site{};
    bool on;
    if (int rc = debug_site(dropout, 0, &site, &on)) return rc;
    if (int rc = check_flash_shape(B, L, 12)) return rc;             // (the int64 L, before it becomes the launcher's int)
    return launch_flash_attn_train(qkv, mask, ctx, stats, B, (int)L, 12, on ? &site : nullptr, (hipStream_t)stream);
}

extern "C" int aspire_debug_flash_attn_train_backward_f32(const float* qkv, const int64_t* mask, const float* ctx, const float* stats,
                                                          const float* dctx, int64_t B, int64_t L, const aspire_bert_dropout* dropout, int layer,
                                                          float* D, float* dqkv, void* stream) {
    ASPIRE_REQUIRE(qkv && mask && ctx && stats && dctx && D && dqkv, ASPIRE_ERR_INVALID_ARG, "null pointer");
    DropSite site{};
    bool on;
    if (int rc = debug_site(dropout, layer, &site, &on)) return rc;
    if (int rc = check_flash_shape(B, L, 12)) return rc;
    return launch_flash_attn_train_backward(qkv, mask, ctx, stats, dctx, D, dqkv, B, (int)L, 12, on ? &site : nullptr, (hipStream_t)stream);
}

extern "C" int aspire_debug_flash_attn_train_packed_f32(const float* qkv, const aspire_bert_packing* packing, int64_t B, int64_t L,
                                                        const aspire_bert_dropout* dropout, float* ctx, float* stats, void* stream) {
    ASPIRE_REQUIRE(qkv && ctx && stats, ASPIRE_ERR_INVALID_ARG, "null pointer");
    DropSite site{};
    bool on;
    if (int rc = debug_site(dropout, 0, &site, &on)) return rc;
    PackedDocs docs{};
    if (int rc = read_packing(packing, B, L, &docs)) return rc;
    if (int rc = check_flash_shape(B, L, 12)) return rc;
    return launch_flash_attn_train_packed(qkv, docs, (int)packing->max_len, ctx, stats, B, 12, on ? &site : nullptr, (hipStream_t)stream);
}

extern "C" int aspire_debug_flash_attn_train_packed_backward_f32(const float* qkv, const aspire_bert_packing* packing, const float* ctx,
                                                                 const float* stats, const float* dctx, int64_t B, int64_t L,
                                                                 const aspire_bert_dropout* dropout, int layer, float* D, float* dqkv,
                                                                 void* stream) {
    ASPIRE_REQUIRE(qkv && ctx && stats && dctx && D && dqkv, ASPIRE_ERR_INVALID_ARG, "null pointer");
    DropSite site{};
    bool on;
    if (int rc = debug_site(dropout, layer, &site, &on)) return rc;
    PackedDocs docs{};
    if (int rc = read_packing(packing, B, L, &docs)) return rc;
    if (int rc = check_flash_shape(B, L, 12)) return rc;
    return launch_flash_attn_train_backward_packed(qkv, docs, (int)packing->max_len, ctx, stats, dctx, D, dqkv, B, 12, on ? &site : nullptr,
                                                   (hipStream_t)stream);
}
