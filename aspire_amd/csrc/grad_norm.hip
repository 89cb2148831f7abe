// The global L2 norm of a set of gradients and torch's clip coefficient from it (torch.nn.utils.clip_grad_norm_), on the device, with
// no host synchronisation: two launches write out[0] = the norm and out[1] = the coefficient, which optim.hip's scaled steps read as
// they load each gradient -- and aspire_grad_scale_f32, the in-place multi-tensor multiply behind aspire_amd.clip_grad_norm_.
//
// Arithmetic.  Every element is squared in double (an fp32 square is exact there) and added in double.  A chunk of kOptimChunk
// elements (multi_tensor.h's chunk list) gives ONE double partial: element j of a chunk belongs to lane (j / 4) % 256, a lane adds
// its elements in ascending j, the 256 lane sums meet in a fixed tree (a butterfly inside each wave, then ((w0 + w1) + (w2 + w3))).
// A second launch of one workgroup adds the partials -- each of its 1024 lanes a strided share in ascending order, then a fixed tree
// -- takes the square root in double and rounds once to fp32.  A double sum of at most 2^27 exact squares is off by at most 2^-26
// relative, so out[0] lies within 1 ulp of float(sqrt(exact sum)).  Because the sum is in double, a gradient of 1e20 does not
// overflow the norm as torch's fp32 sum of squares does: a deliberate departure from torch.
//
//   out[1] = clamp((1 / (out[0] + 1e-6f)) * (float)max_norm, max = 1)   in fp32, every operation rounded once: what torch's
//            clip_grads_with_norm_ computes (`max_norm / tensor` is tensor.reciprocal() * max_norm there).  NaN stays NaN, an
//            infinite norm gives 0.
//
// Determinism.  One partial per chunk, not per workgroup, so the bits do not depend on the grid; the lane that owns an element and
// the order of its additions are the same on the 16-byte path and on the scalar path (a tensor off the 16-byte grid), so they do
// not depend on where a gradient's storage starts; no atomics, one writer per word, the same bits on every run.
//
// Workspace: the table (one 32-byte record per tensor + the prefix sums, as in grad_bucket.hip), then one double per chunk.
#include <math.h>

#include "multi_tensor.h"

namespace aspire {
namespace {

struct alignas(16) NormRec {
    float* g;
    int64_t n;
    int32_t vec;        // 1: g is 16-byte aligned
    int32_t pad[3];
};
static_assert(sizeof(NormRec) == 32, "one record per 32 bytes of the workspace");

constexpr int kFinalLanes = 1024;

size_t table_bytes(int64_t n_tensors) {
    const size_t raw = (size_t)n_tensors * sizeof(NormRec) + (size_t)(n_tensors + 1) * sizeof(int32_t);
    return (raw + 15) & ~(size_t)15;
}

__device__ __forceinline__ void add_sq(double& acc, float x) {
    const double d = (double)x;
    acc = fma(d, d, acc);       // d * d is exact: one rounding, the addition's
}

__global__ void __launch_bounds__(256) grad_sumsq_kernel(const NormRec* __restrict__ recs, const int32_t* __restrict__ prefix,
                                                         int n_tensors, int total_chunks, double* __restrict__ partials) {
    __shared__ double wave_sum[2][4];
    const int tid = threadIdx.x;
    int par = 0;
    for (int c = blockIdx.x; c < total_chunks; c += gridDim.x, par ^= 1) {
        const int t = chunk_tensor(prefix, n_tensors, c);
        const NormRec r = recs[t];
        const int64_t off = (int64_t)(c - prefix[t]) * kOptimChunk;
        const int64_t left = r.n - off;
        const int cnt = left < kOptimChunk ? (int)left : kOptimChunk;
        const float* g = r.g + off;
        double acc = 0.0;
        if (r.vec && cnt == kOptimChunk) {
            constexpr int U = kOptimChunk / (4 * 256);
            float4 G[U];
#pragma unroll
            for (int u = 0; u < U; ++u) G[u] = ld4_stream(g + 4 * (tid + 256 * u));
#pragma unroll
            for (int u = 0; u < U; ++u) {
                add_sq(acc, G[u].x);
                add_sq(acc, G[u].y);
                add_sq(acc, G[u].z);
                add_sq(acc, G[u].w);
            }
        } else {
            // the same lane owns the same elements and adds them in the same order as above
            for (int q = tid; 4 * q < cnt; q += 256) {
                const int j = 4 * q;
                if (r.vec && j + 4 <= cnt) {
                    const float4 G = ld4_stream(g + j);
                    add_sq(acc, G.x);
                    add_sq(acc, G.y);
                    add_sq(acc, G.z);
                    add_sq(acc, G.w);
                } else {
                    const int m = cnt - j < 4 ? cnt - j : 4;
                    for (int e = 0; e < m; ++e) add_sq(acc, g[j + e]);
                }
            }
        }
#pragma unroll
        for (int s = 1; s < 64; s <<= 1) acc += __shfl_xor(acc, s, 64);
        if ((tid & 63) == 0) wave_sum[par][tid >> 6] = acc;
        __syncthreads();
        // (the next chunk writes the other half of wave_sum; this half is written again only behind the next barrier)
        if (tid == 0) partials[c] = (wave_sum[par][0] + wave_sum[par][1]) + (wave_sum[par][2] + wave_sum[par][3]);
    }
}

__global__ void __launch_bounds__(kFinalLanes) grad_norm_final_kernel(const double* __restrict__ partials, int n_partials, float max_norm,
                                                                      float* __restrict__ out) {
    __shared__ double sh[kFinalLanes];
    const int tid = threadIdx.x;
    double acc = 0.0;
    for (int i = tid; i < n_partials; i += kFinalLanes) acc += partials[i];
    sh[tid] = acc;
    __syncthreads();
    for (int s = kFinalLanes / 2; s > 0; s >>= 1) {
        if (tid < s) sh[tid] += sh[tid + s];
        __syncthreads();
    }
    if (tid == 0) {
#pragma clang fp contract(off)
        const float norm = (float)sqrt(sh[0]);
        const float coef = (1.0f / (norm + 1e-6f)) * max_norm;
        out[0] = norm;
        out[1] = coef > 1.0f ? 1.0f : coef;      // (NaN compares false and stays)
    }
}

__device__ __forceinline__ float scaled(float g, float s) {
#pragma clang fp contract(off)
    return g * s;
}

__global__ void __launch_bounds__(256) grad_scale_kernel(const NormRec* __restrict__ recs, const int32_t* __restrict__ prefix, int n_tensors,
                                                         int total_chunks, const float* __restrict__ scale) {
    const int tid = threadIdx.x;
    const float s = *scale;
    for (int c = blockIdx.x; c < total_chunks; c += gridDim.x) {
        const int t = chunk_tensor(prefix, n_tensors, c);
        const NormRec r = recs[t];
        const int64_t off = (int64_t)(c - prefix[t]) * kOptimChunk;
        const int64_t left = r.n - off;
        const int cnt = left < kOptimChunk ? (int)left : kOptimChunk;
        float* g = r.g + off;
        if (r.vec) {
            float4* g4 = reinterpret_cast<float4*>(g);
            const int cnt4 = cnt >> 2;
            for (int i = tid; i < cnt4; i += 256) {
                const float4 G = g4[i];
                g4[i] = make_float4(scaled(G.x, s), scaled(G.y, s), scaled(G.z, s), scaled(G.w, s));
            }
            const int i = 4 * cnt4 + tid;       // the tail of 1-3 elements
            if (i < cnt) g[i] = scaled(g[i], s);
        } else {
            for (int i = tid; i < cnt; i += 256) g[i] = scaled(g[i], s);
        }
    }
}

// the checks both entries share; -> the number of chunks in *chunks
int check_tensors(const char* who, const aspire_grad_tensor* tensors, int64_t n_tensors, int64_t* chunks) {
    ASPIRE_REQUIRE(n_tensors >= 0, ASPIRE_ERR_INVALID_ARG, "%s: n_tensors = %lld is negative", who, (long long)n_tensors);
    ASPIRE_REQUIRE(tensors || n_tensors == 0, ASPIRE_ERR_INVALID_ARG, "%s: null tensor table with n_tensors = %lld", who,
                   (long long)n_tensors);
    *chunks = 0;
    for (int64_t i = 0; i < n_tensors; ++i) {
        const aspire_grad_tensor& t = tensors[i];
        ASPIRE_REQUIRE(t.n >= 0, ASPIRE_ERR_INVALID_ARG, "%s: tensor %lld has n = %lld", who, (long long)i, (long long)t.n);
        ASPIRE_REQUIRE(((uintptr_t)t.grad & 3) == 0, ASPIRE_ERR_INVALID_ARG, "%s: tensor %lld has a gradient pointer that is not 4-byte aligned",
                       who, (long long)i);
        if (t.grad) *chunks += chunks_of(t.n);
        ASPIRE_REQUIRE(*chunks < ((int64_t)1 << 31), ASPIRE_ERR_UNSUPPORTED, "%s: more than 2^31 chunks of %d elements", who, kOptimChunk);
    }
    return ASPIRE_OK;
}

int check_workspace(const char* who, const void* ws, size_t ws_bytes, size_t need) {
    ASPIRE_REQUIRE(ws, ASPIRE_ERR_INVALID_ARG, "%s: null workspace (%zu bytes are needed)", who, need);
    ASPIRE_REQUIRE(ws_bytes >= need, ASPIRE_ERR_INVALID_ARG, "%s: workspace of %zu bytes is too small, need %zu", who, ws_bytes, need);
    ASPIRE_REQUIRE(((uintptr_t)ws & 15) == 0, ASPIRE_ERR_INVALID_ARG, "%s: workspace is not 16-byte aligned", who);
    return ASPIRE_OK;
}

// the table of the tensors that have a gradient, through the staging ring into ws; -> the number of chunks in *total
int upload_table(const char* who, const aspire_grad_tensor* tensors, int64_t n_tensors, void* ws, hipStream_t st, int32_t* total) {
    Staging staging;
    if (const int rc = staging.acquire(who, table_bytes(n_tensors))) return rc;
    NormRec* recs = static_cast<NormRec*>(staging.host());
    int32_t* prefix = reinterpret_cast<int32_t*>(recs + n_tensors);
    int32_t at = 0;
    for (int64_t i = 0; i < n_tensors; ++i) {
        const aspire_grad_tensor& t = tensors[i];
        NormRec r = {};
        r.g = const_cast<float*>(t.grad);
        r.n = t.grad ? t.n : 0;
        r.vec = ((uintptr_t)t.grad & 15) == 0;
        recs[i] = r;
        prefix[i] = at;
        at += (int32_t)chunks_of(r.n);
    }
    prefix[n_tensors] = at;
    *total = at;
    return staging.commit(ws, st);
}

}  // namespace
}  // namespace aspire

extern "C" size_t aspire_grad_norm_workspace_bytes(const int64_t* n, int64_t n_tensors) {
    if (n_tensors < 0 || (n_tensors > 0 && !n)) return 0;
    int64_t chunks = 0;
    for (int64_t i = 0; i < n_tensors; ++i) {
        if (n[i] < 0) return 0;
        chunks += aspire::chunks_of(n[i]);
    }
    const size_t raw = aspire::table_bytes(n_tensors) + (size_t)chunks * sizeof(double);
    return (raw + 15) & ~(size_t)15;
}

extern "C" int aspire_grad_norm_f32(const aspire_grad_tensor* tensors, int64_t n_tensors, double max_norm, float* out, void* workspace,
                                    size_t workspace_bytes, void* stream) {
    using namespace aspire;
    const char* who = "aspire_grad_norm_f32";
    ASPIRE_REQUIRE(isfinite(max_norm) && isfinite((float)max_norm) && (float)max_norm > 0.f, ASPIRE_ERR_INVALID_ARG,
                   "%s: max_norm = %g must be a finite float above 0", who, max_norm);
    ASPIRE_REQUIRE(out, ASPIRE_ERR_INVALID_ARG, "%s: out is null", who);
    ASPIRE_REQUIRE(((uintptr_t)out & 3) == 0, ASPIRE_ERR_INVALID_ARG, "%s: out is not 4-byte aligned", who);
    int64_t chunks = 0;
    if (const int rc = check_tensors(who, tensors, n_tensors, &chunks)) return rc;
    const size_t table = table_bytes(n_tensors);
    const size_t need = (table + (size_t)chunks * sizeof(double) + 15) & ~(size_t)15;
    if (const int rc = check_workspace(who, workspace, workspace_bytes, need)) return rc;

    hipStream_t st = static_cast<hipStream_t>(stream);
    double* partials = reinterpret_cast<double*>(static_cast<char*>(workspace) + table);
    if (chunks > 0) {
        int32_t at = 0;
        if (const int rc = upload_table(who, tensors, n_tensors, workspace, st, &at)) return rc;
        const NormRec* d_recs = static_cast<const NormRec*>(workspace);
        const int32_t* d_prefix = reinterpret_cast<const int32_t*>(d_recs + n_tensors);
        const unsigned grid = (unsigned)(at < kOptimMaxGrid ? at : kOptimMaxGrid);
        hipLaunchKernelGGL(grad_sumsq_kernel, dim3(grid), dim3(256), 0, st, d_recs, d_prefix, (int)n_tensors, (int)at, partials);
        ASPIRE_LAUNCH_OK();
    }
    // no gradient anywhere: the norm of no elements is 0 (torch's value), the coefficient follows from it
    hipLaunchKernelGGL(grad_norm_final_kernel, dim3(1), dim3(kFinalLanes), 0, st, partials, (int)chunks, (float)max_norm, out);
    ASPIRE_LAUNCH_OK();
    return ASPIRE_OK;
}

extern "C" size_t aspire_grad_scale_workspace_bytes(int64_t n_tensors) { return n_tensors > 0 ? aspire::table_bytes(n_tensors) : 16; }

extern "C" int aspire_grad_scale_f32(const aspire_grad_tensor* tensors, int64_t n_tensors, const float* scale, void* workspace,
                                     size_t workspace_bytes, void* stream) {
    using namespace aspire;
    const char* who = "aspire_grad_scale_f32";
    ASPIRE_REQUIRE(scale, ASPIRE_ERR_INVALID_ARG, "%s: scale is null", who);
    ASPIRE_REQUIRE(((uintptr_t)scale & 3) == 0, ASPIRE_ERR_INVALID_ARG, "%s: scale is not 4-byte aligned", who);
    int64_t chunks = 0;
    if (const int rc = check_tensors(who, tensors, n_tensors, &chunks)) return rc;
    if (const int rc = check_workspace(who, workspace, workspace_bytes, n_tensors > 0 ? table_bytes(n_tensors) : 16)) return rc;
    if (chunks == 0) return ASPIRE_OK;

    hipStream_t st = static_cast<hipStream_t>(stream);
    int32_t at = 0;
    if (const int rc = upload_table(who, tensors, n_tensors, workspace, st, &at)) return rc;
    const NormRec* d_recs = static_cast<const NormRec*>(workspace);
    const int32_t* d_prefix = reinterpret_cast<const int32_t*>(d_recs + n_tensors);
    const unsigned grid = (unsigned)(at < kOptimMaxGrid ? at : kOptimMaxGrid);
    hipLaunchKernelGGL(grad_scale_kernel, dim3(grid), dim3(256), 0, st, d_recs, d_prefix, (int)n_tensors, (int)at, scale);
    ASPIRE_LAUNCH_OK();
    return ASPIRE_OK;
}
