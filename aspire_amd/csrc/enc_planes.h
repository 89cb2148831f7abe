// The fp16-plane ("P") layout of the encoder's pre-split GEMM operands: its constants and the device helpers that write and read it.
// Header only.  Users: the epilogues of the P-layout GEMMs (enc_gemm_p.hip) and of the fused attention kernels (enc_attn.hip), the
// row-wise kernels (enc_rows.hip: layernorm_kernel, embed_layernorm_kernel, cls_tap_kernel), cls_attn_kernel, and the host's
// workspace sizes (encoder.hip: carve, plane_offsets).
#pragma once
#include "common.h"

namespace aspire {
namespace {

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

}  // namespace
}  // namespace aspire
