// The gradient bucket of data-parallel training: every gradient of a step packed, scaled by 1 / world, into ONE flat fp32 buffer that
// a single all-reduce then sums and the optimizer step reads in place (aspire_amd/ddp.py: GradReducer).  torch's reducer does the same
// arithmetic per bucket view, mul_out(bucket_view, grad, 1 / world); here it is one launch over all tensors, in the frame of
// optim.hip's step.
//
// Layout (aspire_grad_bucket_elems is its one definition).  Tensor i takes [off_i, off_i + n_i) with off_0 = 0 and
// off_{i+1} = off_i + round_up(n_i, 4): every region starts on a 16-byte boundary of a 16-byte aligned buffer.  Behind the last region
// a tail of round_up(n_tensors, 4) floats says which tensors had a gradient on this rank: 1.0f / 0.0f, unscaled, so that the all-reduce
// leaves the number of ranks that had one.
//
// One launch writes every element of [flat, flat + flat_elems) exactly once: a gradient's elements times (float)scale, zeros for an
// absent gradient, zeros in the pads, the flags and their pad.  No atomics, no zero fill in front, nothing outside the range, the same
// bits on every run.
//
// Work mapping.  multi_tensor.h's chunk list over the padded regions plus the tail as one more entry; a workgroup of 256 lanes takes
// a chunk of kOptimChunk elements as 16-byte slots.  The destination of every slot is 16-byte aligned by the layout, so every store is
// a 16-byte one.  A source that is 16-byte aligned is read with 16-byte streaming loads (it is read once); any other source (a view at
// an odd storage offset) and a region's last 1-3 elements are read element by element into the slot.  The product is one fp32
// multiply with contraction off on both paths: the bits do not depend on where a gradient's storage starts.
#include <math.h>

#include "multi_tensor.h"

namespace aspire {
namespace {

struct alignas(16) PackRec {
    const float* g;     // NULL: no gradient on this rank
    int64_t n;
    int64_t off;        // the region's first element in flat (a multiple of 4)
    int32_t vec;        // 1: g is 16-byte aligned
    int32_t pad;
};
static_assert(sizeof(PackRec) == 32, "one record per 32 bytes of the workspace");

int64_t round4(int64_t n) { return (n + 3) & ~(int64_t)3; }

// records of the n tensors, then n + 2 prefix sums: the tail is entry n of the chunk list
size_t table_bytes(int64_t n_tensors) {
    const size_t raw = (size_t)n_tensors * sizeof(PackRec) + (size_t)(n_tensors + 2) * sizeof(int32_t);
    return (raw + 15) & ~(size_t)15;
}

__device__ __forceinline__ float scaled(float g, float s) {
#pragma clang fp contract(off)
    return g * s;
}

// elements [j, j + 4) of a region whose gradient has n elements, read one by one; beyond n: the pad's zeros
__device__ __forceinline__ float4 quad_scalar(const float* g, int64_t j, int64_t n, float s) {
    float4 v;
    v.x = j + 0 < n ? scaled(g[j + 0], s) : 0.f;
    v.y = j + 1 < n ? scaled(g[j + 1], s) : 0.f;
    v.z = j + 2 < n ? scaled(g[j + 2], s) : 0.f;
    v.w = j + 3 < n ? scaled(g[j + 3], s) : 0.f;
    return v;
}

__global__ void __launch_bounds__(256) grad_pack_kernel(const PackRec* __restrict__ recs, const int32_t* __restrict__ prefix,
                                                        int n_tensors, int total_chunks, float* __restrict__ flat, int64_t tail,
                                                        float s) {
    const int tid = threadIdx.x;
    for (int c = blockIdx.x; c < total_chunks; c += gridDim.x) {
        const int t = chunk_tensor(prefix, n_tensors + 1, c);
        const int64_t off = (int64_t)(c - prefix[t]) * kOptimChunk;     // within the region
        if (t == n_tensors) {
            // the tail: flag j of tensor j, zeros from n_tensors to round_up(n_tensors, 4)
            const int64_t len = ((int64_t)n_tensors + 3) & ~(int64_t)3;
            const int64_t left = len - off;
            const int quads = (int)((left < kOptimChunk ? left : kOptimChunk) >> 2);
            float4* out = reinterpret_cast<float4*>(flat + tail + off);
            for (int q = tid; q < quads; q += 256) {
                const int64_t j = off + 4 * (int64_t)q;
                float4 v;
                v.x = j + 0 < n_tensors && recs[j + 0].g ? 1.f : 0.f;
                v.y = j + 1 < n_tensors && recs[j + 1].g ? 1.f : 0.f;
                v.z = j + 2 < n_tensors && recs[j + 2].g ? 1.f : 0.f;
                v.w = j + 3 < n_tensors && recs[j + 3].g ? 1.f : 0.f;
                out[q] = v;
            }
            continue;
        }
        const PackRec r = recs[t];
        const int64_t left = r.n - off;                                  // >= 1: the chunk exists
        const int cnt = left < kOptimChunk ? (int)left : kOptimChunk;    // gradient elements of this chunk
        const int quads = (cnt + 3) >> 2;                                // 16-byte slots of the region, pad included
        float4* out = reinterpret_cast<float4*>(flat + r.off + off);
        if (!r.g) {
            for (int q = tid; q < quads; q += 256) out[q] = make_float4(0.f, 0.f, 0.f, 0.f);
        } else if (r.vec) {
            const float* g = r.g + off;
            if (cnt == kOptimChunk) {
                constexpr int U = kOptimChunk / (4 * 256);
                float4 G[U];
#pragma unroll
                for (int u = 0; u < U; ++u) G[u] = ld4_stream(g + 4 * (tid + 256 * u));
#pragma unroll
                for (int u = 0; u < U; ++u)
                    out[tid + 256 * u] = make_float4(scaled(G[u].x, s), scaled(G[u].y, s), scaled(G[u].z, s), scaled(G[u].w, s));
            } else {
                const int full = cnt >> 2;
                for (int q = tid; q < full; q += 256) {
                    const float4 G = ld4_stream(g + 4 * q);
                    out[q] = make_float4(scaled(G.x, s), scaled(G.y, s), scaled(G.z, s), scaled(G.w, s));
                }
                if (tid == 0 && full < quads) out[full] = quad_scalar(g, 4 * (int64_t)full, cnt, s);     // 1-3 elements + the pad
            }
        } else {
            const float* g = r.g + off;
            for (int q = tid; q < quads; q += 256) out[q] = quad_scalar(g, 4 * (int64_t)q, cnt, s);
        }
    }
}

}  // namespace
}  // namespace aspire

extern "C" int64_t aspire_grad_bucket_elems(const int64_t* n, int64_t n_tensors, int64_t* offsets) {
    if (n_tensors < 0 || (n_tensors > 0 && !n)) return -1;
    int64_t at = 0;
    for (int64_t i = 0; i < n_tensors; ++i) {
        if (n[i] < 0) return -1;
        if (offsets) offsets[i] = at;
        at += aspire::round4(n[i]);
    }
    return at + aspire::round4(n_tensors);
}

extern "C" size_t aspire_grad_bucket_workspace_bytes(int64_t n_tensors) { return n_tensors > 0 ? aspire::table_bytes(n_tensors) : 16; }

extern "C" int aspire_grad_bucket_pack_f32(const aspire_grad_tensor* tensors, int64_t n_tensors, double scale, float* flat,
                                           int64_t flat_elems, void* workspace, size_t workspace_bytes, void* stream) {
    using namespace aspire;
    const char* who = "aspire_grad_bucket_pack_f32";
    ASPIRE_REQUIRE(n_tensors >= 0, ASPIRE_ERR_INVALID_ARG, "%s: n_tensors = %lld is negative", who, (long long)n_tensors);
    ASPIRE_REQUIRE(n_tensors < ((int64_t)1 << 31) - 4, ASPIRE_ERR_UNSUPPORTED, "%s: n_tensors = %lld is beyond 2^31 - 4", who,
                   (long long)n_tensors);
    ASPIRE_REQUIRE(tensors || n_tensors == 0, ASPIRE_ERR_INVALID_ARG, "%s: null tensor table with n_tensors = %lld", who,
                   (long long)n_tensors);
    ASPIRE_REQUIRE(isfinite(scale) && isfinite((float)scale), ASPIRE_ERR_INVALID_ARG, "%s: scale = %g is not a finite float", who, scale);
    ASPIRE_REQUIRE(flat, ASPIRE_ERR_INVALID_ARG, "%s: flat is null", who);
    ASPIRE_REQUIRE(((uintptr_t)flat & 15) == 0, ASPIRE_ERR_INVALID_ARG, "%s: flat is not 16-byte aligned", who);
    int64_t total = 0, chunks = 0;
    for (int64_t i = 0; i < n_tensors; ++i) {
        const aspire_grad_tensor& t = tensors[i];
        ASPIRE_REQUIRE(t.n >= 0, ASPIRE_ERR_INVALID_ARG, "%s: tensor %lld has n = %lld", who, (long long)i, (long long)t.n);
        ASPIRE_REQUIRE(((uintptr_t)t.grad & 3) == 0, ASPIRE_ERR_INVALID_ARG, "%s: tensor %lld has a gradient pointer that is not 4-byte aligned",
                       who, (long long)i);
        total += round4(t.n);
        chunks += chunks_of(t.n);
        ASPIRE_REQUIRE(chunks < ((int64_t)1 << 30), ASPIRE_ERR_UNSUPPORTED, "%s: more than 2^30 chunks of %d elements", who, kOptimChunk);
    }
    const int64_t tail = total;
    total += round4(n_tensors);
    chunks += chunks_of(round4(n_tensors));
    ASPIRE_REQUIRE(flat_elems == total, ASPIRE_ERR_INVALID_ARG, "%s: flat_elems = %lld, but aspire_grad_bucket_elems gives %lld", who,
                   (long long)flat_elems, (long long)total);
    const uintptr_t f_lo = (uintptr_t)flat, f_hi = f_lo + (uintptr_t)total * sizeof(float);
    for (int64_t i = 0; i < n_tensors; ++i) {
        const aspire_grad_tensor& t = tensors[i];
        if (!t.grad || t.n == 0) continue;
        const uintptr_t g_lo = (uintptr_t)t.grad, g_hi = g_lo + (uintptr_t)t.n * sizeof(float);
        ASPIRE_REQUIRE(g_hi <= f_lo || g_lo >= f_hi, ASPIRE_ERR_INVALID_ARG,
                       "%s: the gradient of tensor %lld overlaps the bucket (was it reduced already? a gradient that lives in the bucket "
                       "cannot be packed into it)", who, (long long)i);
    }
    const size_t need = n_tensors > 0 ? table_bytes(n_tensors) : 16;
    ASPIRE_REQUIRE(workspace, ASPIRE_ERR_INVALID_ARG, "%s: null workspace (aspire_grad_bucket_workspace_bytes(%lld) = %zu)", who,
                   (long long)n_tensors, need);
    ASPIRE_REQUIRE(workspace_bytes >= need, ASPIRE_ERR_INVALID_ARG, "%s: workspace of %zu bytes is too small, need %zu", who, workspace_bytes,
                   need);
    ASPIRE_REQUIRE(((uintptr_t)workspace & 15) == 0, ASPIRE_ERR_INVALID_ARG, "%s: workspace is not 16-byte aligned", who);
    if (chunks == 0) return ASPIRE_OK;      // n_tensors == 0: the bucket has no element

    hipStream_t st = static_cast<hipStream_t>(stream);
    Staging staging;
    if (const int rc = staging.acquire(who, need)) return rc;
    PackRec* recs = static_cast<PackRec*>(staging.host());
    int32_t* prefix = reinterpret_cast<int32_t*>(recs + n_tensors);
    int32_t at = 0;
    int64_t off = 0;
    for (int64_t i = 0; i < n_tensors; ++i) {
        const aspire_grad_tensor& t = tensors[i];
        PackRec r = {};
        r.g = t.grad;
        r.n = t.n;
        r.off = off;
        r.vec = ((uintptr_t)t.grad & 15) == 0;
        recs[i] = r;
        prefix[i] = at;
        at += (int32_t)chunks_of(t.n);
        off += round4(t.n);
    }
    prefix[n_tensors] = at;
    at += (int32_t)chunks_of(round4(n_tensors));
    prefix[n_tensors + 1] = at;
    if (const int rc = staging.commit(workspace, st)) return rc;

    const PackRec* d_recs = static_cast<const PackRec*>(workspace);
    const int32_t* d_prefix = reinterpret_cast<const int32_t*>(d_recs + n_tensors);
    const unsigned grid = (unsigned)(at < kOptimMaxGrid ? at : kOptimMaxGrid);
    hipLaunchKernelGGL(grad_pack_kernel, dim3(grid), dim3(256), 0, st, d_recs, d_prefix, (int)n_tensors, (int)at, flat, tail,
                       (float)scale);
    ASPIRE_LAUNCH_OK();
    return ASPIRE_OK;
}
