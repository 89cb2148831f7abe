// The padding-free training mode's gather and scatter (encoder_bwd.hip runs them at the two ends of a packed call): between the padded
// layout [B L, 768], which the caller's emb_sum, hidden_out, grad_hidden and grad_emb_sum keep, and the packed one [rows, 768] of the
// valid tokens alone, in which the layer stack, its tape and its workspace run.
//
// Kernels (bandwidth-bound row copies: one wave per row of 768, three 16-byte accesses per lane, four rows per workgroup)
//   pack_rows_kernel     out[m, :] = src[row_src[m], :], m < rows
//   unpack_rows_kernel   out[p, :] = src[row_dst[p], :] where row_dst[p] >= 0, exact zeros elsewhere, p < padded_rows: every padded row is
//                        written once, by its own wave, so no zero fill runs in front
// No atomics, one writer per element.  The lists are the caller's device memory: an index outside its tensor is never followed (pack:
// clamped; unpack: the row is zeros).
#include "enc_types.h"

namespace aspire {
namespace {

constexpr int kPackRows = 4;        // rows (waves) per workgroup

__global__ void __launch_bounds__(64 * kPackRows) pack_rows_kernel(const float* __restrict__ src, const int32_t* __restrict__ row_src,
                                                                   float* __restrict__ out, int64_t rows, int64_t padded_rows) {
    const int lane = threadIdx.x & 63;
    const int64_t m = (int64_t)blockIdx.x * kPackRows + (threadIdx.x >> 6);
    if (m >= rows) return;
    const int64_t p = min(max((int64_t)row_src[m], (int64_t)0), padded_rows - 1);
    const float4* s = reinterpret_cast<const float4*>(src + (size_t)p * kD);
    float4* o = reinterpret_cast<float4*>(out + (size_t)m * kD);
    const float4 a = s[lane], b = s[lane + 64], c = s[lane + 128];
    o[lane] = a;
    o[lane + 64] = b;
    o[lane + 128] = c;
}

__global__ void __launch_bounds__(64 * kPackRows) unpack_rows_kernel(const float* __restrict__ src, const int32_t* __restrict__ row_dst,
                                                                     float* __restrict__ out, int64_t padded_rows, int64_t rows) {
    const int lane = threadIdx.x & 63;
    const int64_t p = (int64_t)blockIdx.x * kPackRows + (threadIdx.x >> 6);
    if (p >= padded_rows) return;
    const int64_t m = row_dst[p];
    float4 a = make_float4(0.f, 0.f, 0.f, 0.f), b = a, c = a;
    if (m >= 0 && m < rows) {                                   // uniform per wave
        const float4* s = reinterpret_cast<const float4*>(src + (size_t)m * kD);
        a = s[lane];
        b = s[lane + 64];
        c = s[lane + 128];
    }
    float4* o = reinterpret_cast<float4*>(out + (size_t)p * kD);
    o[lane] = a;
    o[lane + 64] = b;
    o[lane + 128] = c;
}

}  // namespace

int launch_pack_rows(const float* src, const int32_t* row_src, float* out, int64_t rows, int64_t padded_rows, hipStream_t st) {
    if (rows <= 0) return ASPIRE_OK;
    hipLaunchKernelGGL(pack_rows_kernel, dim3((unsigned)((rows + kPackRows - 1) / kPackRows)), dim3(64 * kPackRows), 0, st, src, row_src, out, rows,
                       padded_rows);
    ASPIRE_LAUNCH_OK();
    return ASPIRE_OK;
}

int launch_unpack_rows(const float* src, const int32_t* row_dst, float* out, int64_t padded_rows, int64_t rows, hipStream_t st) {
    if (padded_rows <= 0) return ASPIRE_OK;
    hipLaunchKernelGGL(unpack_rows_kernel, dim3((unsigned)((padded_rows + kPackRows - 1) / kPackRows)), dim3(64 * kPackRows), 0, st, src, row_dst,
                       out, padded_rows, rows);
    ASPIRE_LAUNCH_OK();
    return ASPIRE_OK;
}

}  // namespace aspire
