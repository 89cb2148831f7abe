// The dropout passes of the encoder under training (encoder_bwd.hip runs them; the contract -- generator, keying, sites, keep rule --
// is dropout_rng.h's).  A mask is never stored: every pass forms its words again from (seed, step, site, logical element index), so the
// backward multiplies by the bits the forward drew.  Bandwidth-bound row kernels, one Philox call per four consecutive elements, no
// atomics, every output element has one writer.
//
// Kernels
//   dropout_flat_kernel     out = keep . scale . (a [+ a2]) [+ res] over a contiguous tensor whose length is a multiple of 4: thread i
//                           owns elements 4 i .. 4 i + 3 = Philox block i, one 16-byte load per operand and one store.  The hidden
//                           sites both ways (forward: z in place + the residual; backward: dz = keep . scale . ds, and at site 0 the
//                           two branches' sum), and the probabilities when L % 4 == 0 (then Lp == L: the tape's rows ARE the logical
//                           tensor).  out may be a.  With a row map (the padding-free mode's packed rows of 768) thread i's block is
//                           the one its elements have in the padded tensor: row_map[row] x 192 + its index in the row.
//   dropout_ragged_kernel   the probabilities when L % 4 != 0: rows of L logical elements in a row stride of Lp.  A thread owns four
//                           padded columns (16-byte aligned in memory); their logical indices row L + j .. + 3 straddle two Philox
//                           blocks unless they happen to start one, so it draws the second block only then.  Pad columns [L, Lp) are
//                           written as zeros.  out may be a.
//   dropout_mask_kernel     keep bytes of elements first .. first + n - 1 of a site (aspire_bert_dropout_mask_u8): how a caller sees a
//                           mask; the same drop_keep as above, one thread per element.
#include "enc_types.h"      // (dropout_rng.h with it)

namespace aspire {
namespace {

__device__ __forceinline__ float drop1(float v, uint32_t word, const DropSite& d) { return word >= d.thr ? v * d.scale : 0.f; }

// MAP (the padding-free mode: packed rows of 768 = 192 Philox blocks): thread i's block is the one its elements have in the PADDED
// tensor, row_map[row] x 192 + the block's index in the row.  MAP = false is the kernel without a map.
template <bool MAP>
__global__ void __launch_bounds__(256) dropout_flat_kernel(const float* a, const float* __restrict__ a2, const float* __restrict__ res,
                                                           float* out, int64_t n4, DropSite d, const int32_t* __restrict__ row_map) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n4) return;
    uint64_t blk = (uint64_t)i;
    if constexpr (MAP) {
        const int64_t row = i / (kD / 4);
        blk = (uint64_t)row_map[row] * (kD / 4) + (uint64_t)(i - row * (kD / 4));
    }
    float4 v = reinterpret_cast<const float4*>(a)[i];
    if (a2) {
        const float4 w = reinterpret_cast<const float4*>(a2)[i];
        v = make_float4(v.x + w.x, v.y + w.y, v.z + w.z, v.w + w.w);
    }
    const Philox4 r = drop_block(d, blk);
    v = make_float4(drop1(v.x, r.w[0], d), drop1(v.y, r.w[1], d), drop1(v.z, r.w[2], d), drop1(v.w, r.w[3], d));
    if (res) {
        const float4 w = reinterpret_cast<const float4*>(res)[i];
        v = make_float4(v.x + w.x, v.y + w.y, v.z + w.z, v.w + w.w);
    }
    reinterpret_cast<float4*>(out)[i] = v;
}

// a, out [rows][ld], ld % 4 == 0, L < ld <= L + 3; cols4 = ld / 4
__global__ void __launch_bounds__(256) dropout_ragged_kernel(const float* a, float* out, int64_t rows, int L, int cols4, DropSite d) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= rows * cols4) return;
    const int64_t row = i / cols4;
    const int j = 4 * (int)(i - row * cols4);
    const float4 v = reinterpret_cast<const float4*>(a)[i];
    const uint64_t e = (uint64_t)row * (uint64_t)L + (uint64_t)j;
    const uint32_t o = (uint32_t)(e & 3);
    const Philox4 r0 = drop_block(d, e >> 2);
    Philox4 r1 = r0;
    if (o) r1 = drop_block(d, (e >> 2) + 1);
    // element e + k takes word o + k of r0, or word o + k - 4 of r1
    const uint32_t w0 = drop_word(r0, o);
    const uint32_t w1 = o + 1 < 4 ? drop_word(r0, o + 1) : drop_word(r1, o - 3);
    const uint32_t w2 = o + 2 < 4 ? drop_word(r0, o + 2) : drop_word(r1, o - 2);
    const uint32_t w3 = o + 3 < 4 ? drop_word(r0, o + 3) : drop_word(r1, o - 1);
    float4 y;
    y.x = j < L ? drop1(v.x, w0, d) : 0.f;
    y.y = j + 1 < L ? drop1(v.y, w1, d) : 0.f;
    y.z = j + 2 < L ? drop1(v.z, w2, d) : 0.f;
    y.w = j + 3 < L ? drop1(v.w, w3, d) : 0.f;
    reinterpret_cast<float4*>(out)[i] = y;
}

__global__ void __launch_bounds__(256) dropout_mask_kernel(unsigned char* __restrict__ keep, uint64_t first, int64_t n, DropSite d) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    keep[i] = drop_keep(d, first + (uint64_t)i) ? 1 : 0;
}

}  // namespace

int launch_dropout_flat(const float* a, const float* a2, const float* res, float* out, int64_t n, const DropSite& d, hipStream_t st,
                        const int32_t* row_map) {
    const int64_t n4 = n / 4;     // (n = rows x 768, or B H L L with L % 4 == 0)
    if (row_map)
        hipLaunchKernelGGL(dropout_flat_kernel<true>, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, st, a, a2, res, out, n4, d, row_map);
    else
        hipLaunchKernelGGL(dropout_flat_kernel<false>, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, st, a, a2, res, out, n4, d, row_map);
    ASPIRE_LAUNCH_OK();
    return ASPIRE_OK;
}

int launch_dropout_probs(const float* p, float* out, int64_t rows, int L, int ld, const DropSite& d, hipStream_t st) {
    if (ld == L) return launch_dropout_flat(p, nullptr, nullptr, out, rows * L, d, st);
    const int64_t n4 = rows * (ld / 4);
    hipLaunchKernelGGL(dropout_ragged_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, st, p, out, rows, L, ld / 4, d);
    ASPIRE_LAUNCH_OK();
    return ASPIRE_OK;
}

int launch_dropout_mask(unsigned char* keep, uint64_t first, int64_t n, const DropSite& d, hipStream_t st) {
    hipLaunchKernelGGL(dropout_mask_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, keep, first, n, d);
    ASPIRE_LAUNCH_OK();
    return ASPIRE_OK;
}

}  // namespace aspire
