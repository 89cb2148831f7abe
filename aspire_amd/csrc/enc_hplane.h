// The single-fp16-plane ("H") layout of the GEMM operands of the inference encoder's opt-in fp16 matmul mode (ASPIRE_MATMUL_FP16):
// its constants and the device helpers that write and read it.  Header only.  Users: enc_gemm_h.hip (the split, the GEMM's epilogue,
// the LayerNorm row kernel) and the host's buffer sizes (encoder.hip).
#pragma once
#include "enc_planes.h"

namespace aspire {
namespace {

// ---------------------------------------------------------------------------------------------------------------------
// The mode's operands: every element rounded to fp16 ONCE (round to nearest even; activations as they are, weights as
// fp16(kPWeightScale w), the factor taken off exactly in the epilogue), ONE v_mfma_f32_32x32x16_f16 per term where the P layout
// (enc_planes.h) pays three, and half the bytes per unit of k.
//
// H layout of a matrix X [R, K] (K % 32 == 0), 2 bytes per element: for every 32-wide k block kb and row r four 16-byte pieces
// q = 0 .. 3 = the 8 fp16 at k = 32 kb + 8 q .. + 7, stored at
//     piece index (kb * R + r) * 4 + (q ^ ((r >> 2) & 3))
// -- the P layout's 64-byte row, its swizzle and its contiguous 8 KB per 128 rows and k block, with "k quarter" where P has
// "(plane, k half)": the LDS-DMA of a k block and the conflict-free ds_read_b128 fragment read carry over unchanged.  A k block is
// TWO MFMA k steps: for step s lane (row, k half lk) reads piece (2 s + lk) ^ ((row >> 2) & 3).
// kPPadRows rows of slack lie behind the matrix, as behind a P matrix: the last row tile reads past R.
// ---------------------------------------------------------------------------------------------------------------------
constexpr int kHRowBytes = 64;                       // one row of one k block: four k quarters x 16 bytes
constexpr int kHBlockK = 32;                         // k per block
constexpr int kHTile = 128 * kHRowBytes;             // 128 rows of one k block (8 KB)

__host__ __device__ inline size_t h_bytes(int64_t R, int64_t K) { return (size_t)(R + kPPadRows) * K * 2; }

__device__ __forceinline__ uint32_t pack2_f16(float x, float y) {
    return (uint32_t)__builtin_bit_cast(uint16_t, (_Float16)x) | ((uint32_t)__builtin_bit_cast(uint16_t, (_Float16)y) << 16);
}

// four consecutive k (k % 4 == 0) of row r: 8 bytes
__device__ __forceinline__ void h_store4(void* H, int64_t R, int64_t r, int k, float x, float y, float z, float w) {
    const int kb = k >> 5, q = (k >> 3) & 3, half = (k >> 2) & 1, sw = (int)((r >> 2) & 3);
    char* row = (char*)H + ((size_t)kb * R + r) * kHRowBytes + half * 8;
    *reinterpret_cast<uint2*>(row + 16 * (q ^ sw)) = make_uint2(pack2_f16(x, y), pack2_f16(z, w));
}
__device__ __forceinline__ float4 h_load4(const void* H, int64_t R, int64_t r, int k) {
    const int kb = k >> 5, q = (k >> 3) & 3, half = (k >> 2) & 1, sw = (int)((r >> 2) & 3);
    const char* row = (const char*)H + ((size_t)kb * R + r) * kHRowBytes + half * 8;
    const uint2 h = *reinterpret_cast<const uint2*>(row + 16 * (q ^ sw));
    typedef _Float16 h2 __attribute__((ext_vector_type(2)));
    const h2 h0 = __builtin_bit_cast(h2, h.x), h1 = __builtin_bit_cast(h2, h.y);
    return make_float4((float)h0.x, (float)h0.y, (float)h1.x, (float)h1.y);
}

// EIGHT consecutive k (k % 8 == 0) of row r: one whole 16-byte piece, at a 32-bit byte offset from the base (an H matrix is far below 4 GB)
__device__ __forceinline__ uint32_t h_slot8(uint32_t R, uint32_t r, uint32_t k) {
    return (((k >> 5) * R + r) << 6) + 16 * (((k >> 3) & 3) ^ ((r >> 2) & 3));
}
__device__ __forceinline__ void h_store8_at(void* H, uint32_t slot, const float (&x)[8]) {
    f16x8_t h;
#pragma unroll
    for (int c = 0; c < 8; ++c) h[c] = (_Float16)x[c];
    *reinterpret_cast<f16x8_t*>((char*)H + slot) = h;
}
__device__ __forceinline__ void h_load8_at(const void* H, uint32_t slot, float (&x)[8]) {
    const f16x8_t h = *reinterpret_cast<const f16x8_t*>((const char*)H + slot);
#pragma unroll
    for (int c = 0; c < 8; ++c) x[c] = (float)h[c];
}

}  // namespace
}  // namespace aspire
