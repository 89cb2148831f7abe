// The row-wise kernels of the encoder's backward (encoder_bwd.hip is the host side: the tape, the layer loops, the C entry points).
//
// Kernels
//   gelu_forward_kernel        a = GELU(u) with the forward's gelu_erf (enc_types.h): the training forward keeps the pre-GELU value on
//                              its tape, so the activation is a pass of its own there                       (one thread per 4 values)
//   gelu_backward_kernel       du = dy (Phi(u) + u phi(u)), Phi(u) = (1 + erf(u / sqrt 2)) / 2, phi(u) = exp(-u^2 / 2) / sqrt(2 pi)
//   softmax_backward_kernel    dS = scale P (dP - sum_j dP_j P_j) over a score row's L <= 512 keys held in registers, in place; the pad
//                              columns [L, ld) are written as zeros (the dQ / dK products run k up to ld)    (one wave per row)
//   layernorm_backward_kernel  the moments are formed again from the saved pre-norm row with layernorm_kernel's arithmetic;
//                              dy = dy (+ dy_res: the residual branch's gradient, added in the same pass);
//                              dx = rstd (g dy - mean(g dy) - xhat mean(g dy xhat)); one wave per row, a workgroup walks 16 rows and
//                              leaves their sums of dy xhat and dy as one row of partials
//   colsum_partial_kernel      sums of 32 rows per column (the bias gradients)                               (one thread per column)
//   colsum_final_kernel        the partials' rows added per column
//                              both as four interleaved chains (row i to chain i % 4) joined pairwise: a quarter of the roundings of
//                              one running sum (which left an FFN2 bias gradient over 288 heavy-tailed rows 4.4 x the fp32 CPU sum's
//                              distance from float64), and four loads in flight
// No atomics: every sum has one writer and a fixed order, so a backward gives the same bits on every run.
#include <math.h>

#include "enc_types.h"

namespace aspire {
namespace {

constexpr int kLnbRows = 16;     // rows per workgroup of layernorm_backward_kernel (4 per wave)
constexpr int kColRows = 32;     // rows per workgroup of colsum_partial_kernel

__global__ void __launch_bounds__(256) gelu_forward_kernel(const float* __restrict__ u, float* __restrict__ a, int64_t n4) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n4) return;
    const float4 v = reinterpret_cast<const float4*>(u)[i];
    reinterpret_cast<float4*>(a)[i] = make_float4(gelu_erf(v.x), gelu_erf(v.y), gelu_erf(v.z), gelu_erf(v.w));
}

__device__ __forceinline__ float gelu_grad(float u) {
    const float cdf = 0.5f * (1.0f + erff(u * 0.70710678118654752440f));
    const float pdf = expf(-0.5f * u * u) * 0.39894228040143267794f;
    return cdf + u * pdf;
}

__global__ void __launch_bounds__(256) gelu_backward_kernel(const float* dy, const float* __restrict__ u, float* du, int64_t n4) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n4) return;
    const float4 g = reinterpret_cast<const float4*>(dy)[i];
    const float4 v = reinterpret_cast<const float4*>(u)[i];
    reinterpret_cast<float4*>(du)[i] = make_float4(g.x * gelu_grad(v.x), g.y * gelu_grad(v.y), g.z * gelu_grad(v.z), g.w * gelu_grad(v.w));
}

// dp [rows][ld] in place, p [rows][ld] the saved probabilities.  A masked key has p == 0 exactly, so its dS is 0 exactly; a row whose
// mask is all zero has uniform p and takes the same formula.
__global__ void __launch_bounds__(256) softmax_backward_kernel(float* __restrict__ dp, const float* __restrict__ p, int64_t rows, int L,
                                                               int ld, float scale) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    float* d = dp + row * ld;
    const float* pr = p + row * ld;
    constexpr int kMaxPer = 8;  // L <= 512
    float pv[kMaxPer], dv[kMaxPer];
    float dot = 0.f;
#pragma unroll
    for (int c = 0; c < kMaxPer; ++c) {
        const int j = lane + 64 * c;
        pv[c] = j < L ? pr[j] : 0.f;
        dv[c] = j < L ? d[j] : 0.f;
        dot = fmaf(dv[c], pv[c], dot);
    }
    dot = wave_sum(dot);
#pragma unroll
    for (int c = 0; c < kMaxPer; ++c) {
        const int j = lane + 64 * c;
        if (j < ld) d[j] = j < L ? scale * (pv[c] * (dv[c] - dot)) : 0.f;
    }
}

// partial [row blocks][2][768]: (sum of dy xhat, sum of dy) over the block's rows, waves added in order 0..3
__global__ void __launch_bounds__(256) layernorm_backward_kernel(const float* __restrict__ x, const float* __restrict__ gamma, float eps,
                                                                 const float* __restrict__ dy, const float* __restrict__ dy_res,
                                                                 float* __restrict__ dx, int64_t rows, float* __restrict__ partial) {
    __shared__ float sm[4][2][kD];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float4 gm[3], ag[3], ab[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        gm[c] = *reinterpret_cast<const float4*>(gamma + 4 * lane + 256 * c);
        ag[c] = make_float4(0.f, 0.f, 0.f, 0.f);
        ab[c] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    for (int i = 0; i < kLnbRows / 4; ++i) {
        const int64_t row = (int64_t)blockIdx.x * kLnbRows + 4 * i + wave;
        if (row >= rows) break;      // (wave-uniform)
        float4 v[3], g[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const size_t o = (size_t)row * kD + 4 * lane + 256 * c;
            v[c] = *reinterpret_cast<const float4*>(x + o);
            g[c] = *reinterpret_cast<const float4*>(dy + o);
            if (dy_res) {
                const float4 r = *reinterpret_cast<const float4*>(dy_res + o);
                g[c] = make_float4(g[c].x + r.x, g[c].y + r.y, g[c].z + r.z, g[c].w + r.w);
            }
        }
        // the forward's moments (layernorm_row, enc_rows.hip), operation for operation
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
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            v[c] = make_float4((v[c].x - mean) * rstd, (v[c].y - mean) * rstd, (v[c].z - mean) * rstd, (v[c].w - mean) * rstd);   // xhat
            ag[c] = make_float4(fmaf(g[c].x, v[c].x, ag[c].x), fmaf(g[c].y, v[c].y, ag[c].y), fmaf(g[c].z, v[c].z, ag[c].z),
                                fmaf(g[c].w, v[c].w, ag[c].w));
            ab[c] = make_float4(ab[c].x + g[c].x, ab[c].y + g[c].y, ab[c].z + g[c].z, ab[c].w + g[c].w);
            g[c] = make_float4(g[c].x * gm[c].x, g[c].y * gm[c].y, g[c].z * gm[c].z, g[c].w * gm[c].w);                           // g dy
            s1 += (g[c].x + g[c].y) + (g[c].z + g[c].w);
            s2 += (g[c].x * v[c].x + g[c].y * v[c].y) + (g[c].z * v[c].z + g[c].w * v[c].w);
        }
        const float m1 = wave_sum(s1) * (1.0f / kD), m2 = wave_sum(s2) * (1.0f / kD);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float4 o;
            o.x = rstd * ((g[c].x - m1) - v[c].x * m2);
            o.y = rstd * ((g[c].y - m1) - v[c].y * m2);
            o.z = rstd * ((g[c].z - m1) - v[c].z * m2);
            o.w = rstd * ((g[c].w - m1) - v[c].w * m2);
            *reinterpret_cast<float4*>(dx + (size_t)row * kD + 4 * lane + 256 * c) = o;
        }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        *reinterpret_cast<float4*>(&sm[wave][0][4 * lane + 256 * c]) = ag[c];
        *reinterpret_cast<float4*>(&sm[wave][1][4 * lane + 256 * c]) = ab[c];
    }
    __syncthreads();
    float* out = partial + (size_t)blockIdx.x * 2 * kD;
    const float* s0 = &sm[0][0][0];
    for (int j = threadIdx.x; j < 2 * kD; j += 256) out[j] = ((s0[j] + s0[2 * kD + j]) + s0[4 * kD + j]) + s0[6 * kD + j];
}

// x [rows][N] -> partial [row blocks][N]: rows added in a fixed order (four chains)
__global__ void __launch_bounds__(256) colsum_partial_kernel(const float* __restrict__ x, int64_t rows, int N, float* __restrict__ partial) {
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n >= N) return;
    const int64_t r0 = (int64_t)blockIdx.y * kColRows;
    const int64_t r1 = r0 + kColRows < rows ? r0 + kColRows : rows;
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
    int64_t r = r0;
    for (; r + 4 <= r1; r += 4) {
        s0 += x[(size_t)r * N + n];
        s1 += x[(size_t)(r + 1) * N + n];
        s2 += x[(size_t)(r + 2) * N + n];
        s3 += x[(size_t)(r + 3) * N + n];
    }
    for (; r < r1; ++r) s0 += x[(size_t)r * N + n];
    partial[(size_t)blockIdx.y * N + n] = (s0 + s1) + (s2 + s3);
}

// partial [parts][N] -> column n < split to out_a[n], the others to out_b[n - split]; parts added in a fixed order (four chains)
__global__ void __launch_bounds__(256) colsum_final_kernel(const float* __restrict__ partial, int parts, int N, float* __restrict__ out_a,
                                                           int split, float* __restrict__ out_b) {
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n >= N) return;
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
    int p = 0;
    for (; p + 4 <= parts; p += 4) {
        s0 += partial[(size_t)p * N + n];
        s1 += partial[(size_t)(p + 1) * N + n];
        s2 += partial[(size_t)(p + 2) * N + n];
        s3 += partial[(size_t)(p + 3) * N + n];
    }
    for (; p < parts; ++p) s0 += partial[(size_t)p * N + n];
    const float s = (s0 + s1) + (s2 + s3);
    if (n < split)
        out_a[n] = s;
    else
        out_b[n - split] = s;
}

}  // namespace

int launch_gelu_forward(const float* u, float* a, int64_t n, hipStream_t st) {
    const int64_t n4 = n / 4;     // (n = rows x ffn_dim, ffn_dim % 64 == 0)
    hipLaunchKernelGGL(gelu_forward_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, st, u, a, n4);
    ASPIRE_LAUNCH_OK();
    return ASPIRE_OK;
}

int launch_gelu_backward(const float* dy, const float* u, float* du, int64_t n, hipStream_t st) {
    const int64_t n4 = n / 4;
    hipLaunchKernelGGL(gelu_backward_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, st, dy, u, du, n4);
    ASPIRE_LAUNCH_OK();
    return ASPIRE_OK;
}

int launch_softmax_backward(float* dp, const float* p, int64_t rows, int L, int ld, float scale, hipStream_t st) {
    hipLaunchKernelGGL(softmax_backward_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, st, dp, p, rows, L, ld, scale);
    ASPIRE_LAUNCH_OK();
    return ASPIRE_OK;
}

size_t layernorm_backward_partial_floats(int64_t rows) { return (size_t)((rows + kLnbRows - 1) / kLnbRows) * 2 * kD; }

int launch_layernorm_backward(const float* x, const float* gamma, float eps, const float* dy, const float* dy_res, float* dx, float* dgamma,
                              float* dbeta, int64_t rows, float* partial, hipStream_t st) {
    const int parts = (int)((rows + kLnbRows - 1) / kLnbRows);
    hipLaunchKernelGGL(layernorm_backward_kernel, dim3((unsigned)parts), dim3(256), 0, st, x, gamma, eps, dy, dy_res, dx, rows, partial);
    ASPIRE_LAUNCH_OK();
    hipLaunchKernelGGL(colsum_final_kernel, dim3(2 * kD / 256), dim3(256), 0, st, partial, parts, 2 * kD, dgamma, kD, dbeta);
    ASPIRE_LAUNCH_OK();
    return ASPIRE_OK;
}

size_t colsum_partial_floats(int64_t rows, int N) { return (size_t)((rows + kColRows - 1) / kColRows) * N; }

int launch_colsum(const float* x, int64_t rows, int N, float* out, float* partial, hipStream_t st) {
    const int parts = (int)((rows + kColRows - 1) / kColRows);
    hipLaunchKernelGGL(colsum_partial_kernel, dim3((unsigned)((N + 255) / 256), (unsigned)parts), dim3(256), 0, st, x, rows, N, partial);
    ASPIRE_LAUNCH_OK();
    hipLaunchKernelGGL(colsum_final_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, st, partial, parts, N, out, N, out);
    ASPIRE_LAUNCH_OK();
    return ASPIRE_OK;
}

}  // namespace aspire
