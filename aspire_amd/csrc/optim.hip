// The parameter update of the reference's trainer (src/learning/trainer.py:178-181: optim.Adam / optim.Adagrad at torch's defaults) as
// ONE launch over every tensor of a parameter set: torch's single-tensor formulas in fp32, one element per lane slot, division and
// square root correctly rounded (hipcc's default; a gradient of 1e-20 squares to a denormal, which the default keeps too).
//
//   Adam      m += (g - m) (1 - b1);  v = v b2 + g g (1 - b2);  p -= step_size (m / (sqrt(v) / bc2_sqrt + eps))
//             step_size = lr / (1 - b1^t), bc2_sqrt = sqrt(1 - b2^t): per tensor, in double on the host, passed as floats
//   Adagrad   s += g g;  p -= clr (g / (sqrt(s) + eps));  clr = lr / (1 + (t - 1) lr_decay)
//   AdamW     p = p (float)(1 - lr weight_decay) in front of Adam's update: one fp32 multiply, the factor per tensor in double on the
//             host (torch's _single_tensor_adam with decoupled_weight_decay=True).  lr and weight_decay are per tensor, so param groups
//             that differ in them alone share a launch.
//   scaled    every rule on g * (*grad_scale), a float on the device read once per workgroup (the clip coefficient of grad_norm.hip):
//             one fp32 multiply, never contracted, in front of the formula -- torch's grad.mul_(clip_coef) followed by the step, the
//             gradients in memory left as they are.
// The plain, scaled and decaying forms are instantiations of one kernel template; the plain ones are what they were before the others
// existed, so aspire_adam_step_f32 / aspire_adagrad_step_f32 keep their launches and their bits.
//
// Work mapping.  A tensor is cut into chunks of kOptimChunk elements (tuning.h); the grid is capped at kOptimMaxGrid workgroups, which
// grid-stride over the global chunk list.  A workgroup finds its (tensor, offset) with a binary search over the prefix sum of chunk
// counts -- wave-uniform, so scalar loads -- and nothing is looked up per element.  The table (one 64-byte record per tensor + the
// prefix sums) lives in the caller's workspace: the host fills a pinned staging slot of the library and copies it there on the call's
// stream, so the caller's descriptor array is dead when the call returns and the call does not wait for the stream.  The chunk list
// and the staging ring are multi_tensor.h's, shared with grad_bucket.hip.
//
// Memory access.  A tensor whose four pointers are 16-byte aligned goes through 16-byte loads and stores (a chunk starts at a multiple
// of 4 elements, so the alignment carries), its last 1-3 elements through a scalar tail; any other tensor (a view at an odd storage
// offset) takes the scalar path throughout.  Every element has one writer, no atomics, nothing outside [ptr, ptr + n) is touched, the
// same bits on every run.  Non-finite gradients propagate as the formulas say.
#include <math.h>

#include <type_traits>

#include "multi_tensor.h"

namespace aspire {
namespace {

constexpr int kAdam = 0, kAdagrad = 1;

struct alignas(16) OptimRec {
    float* p;
    const float* g;
    float* s1;      // exp_avg | sum
    float* s2;      // exp_avg_sq | unused
    int64_t n;
    float a;        // step_size | clr
    float b;        // bc2_sqrt | unused
    int32_t vec;    // 1: the four pointers are 16-byte aligned
    float d;        // AdamW's decay factor 1 - lr * weight_decay | unused
    int32_t pad[2];
};
static_assert(sizeof(OptimRec) == 64, "one record per 64 bytes of the workspace");

struct OptimCoef {
    float w1, b2, w2, eps;      // 1 - b1, b2, 1 - b2 (Adam); eps (both)
};

size_t table_bytes(int64_t n_tensors) {
    const size_t raw = (size_t)n_tensors * sizeof(OptimRec) + (size_t)(n_tensors + 1) * sizeof(int32_t);
    return (raw + 15) & ~(size_t)15;
}

// SCALED: the gradient is multiplied by gs first (one fp32 multiply: torch's grad.mul_(clip_coef) in front of the step); DECAY: the
// parameter by d (one fp32 multiply: torch's param.mul_(1 - lr * weight_decay) of decoupled weight decay).  Without either the
// function is the plain step's, instruction for instruction.
template <int RULE, bool SCALED, bool DECAY>
__device__ __forceinline__ void update1(float& p, float g, float& s1, float& s2, float a, float b, float gs, float d, const OptimCoef& k) {
    // the fused multiply-adds are written out and the compiler forms no others: the vector path, the tails and the scalar path then
    // round alike, so a tensor's bits do not depend on where its storage starts
#pragma clang fp contract(off)
    if constexpr (SCALED) g = g * gs;
    if constexpr (DECAY) p = p * d;
    if constexpr (RULE == kAdam) {
        s1 = fmaf(g - s1, k.w1, s1);
        s2 = fmaf(g * g, k.w2, s2 * k.b2);
        p = fmaf(-a, s1 / (sqrtf(s2) / b + k.eps), p);
    } else {
        s1 = fmaf(g, g, s1);
        p = fmaf(-a, g / (sqrtf(s1) + k.eps), p);
    }
}

template <int RULE, bool SCALED, bool DECAY>
__device__ __forceinline__ void update4(float4& p, const float4& g, float4& s1, float4& s2, float a, float b, float gs, float d,
                                        const OptimCoef& k) {
    update1<RULE, SCALED, DECAY>(p.x, g.x, s1.x, s2.x, a, b, gs, d, k);
    update1<RULE, SCALED, DECAY>(p.y, g.y, s1.y, s2.y, a, b, gs, d, k);
    update1<RULE, SCALED, DECAY>(p.z, g.z, s1.z, s2.z, a, b, gs, d, k);
    update1<RULE, SCALED, DECAY>(p.w, g.w, s1.w, s2.w, a, b, gs, d, k);
}

template <int RULE, bool SCALED, bool DECAY>
__global__ void __launch_bounds__(256) optim_step_kernel(const OptimRec* __restrict__ recs, const int32_t* __restrict__ prefix,
                                                         int n_tensors, int total_chunks, OptimCoef k,
                                                         const float* __restrict__ grad_scale) {
    const int tid = threadIdx.x;
    float gs = 1.f;
    if constexpr (SCALED) gs = *grad_scale;     // once per workgroup
    for (int c = blockIdx.x; c < total_chunks; c += gridDim.x) {
        const int t = chunk_tensor(prefix, n_tensors, c);
        const OptimRec r = recs[t];
        const int64_t off = (int64_t)(c - prefix[t]) * kOptimChunk;
        const int64_t left = r.n - off;
        const int cnt = left < kOptimChunk ? (int)left : kOptimChunk;
        float* p = r.p + off;
        const float* g = r.g + off;
        float* s1 = r.s1 + off;
        float* s2 = RULE == kAdam ? r.s2 + off : nullptr;
        if (r.vec) {
            float4* p4 = reinterpret_cast<float4*>(p);
            const float4* g4 = reinterpret_cast<const float4*>(g);
            float4* s14 = reinterpret_cast<float4*>(s1);
            float4* s24 = reinterpret_cast<float4*>(s2);
            if (cnt == kOptimChunk) {
                constexpr int U = kOptimChunk / (4 * 256);
                float4 P[U], G[U], A[U], B[U];
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const int i = tid + 256 * u;
                    G[u] = ld4_stream(g + 4 * i);
                    P[u] = p4[i];
                    A[u] = s14[i];
                    B[u] = RULE == kAdam ? s24[i] : make_float4(0.f, 0.f, 0.f, 0.f);
                }
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const int i = tid + 256 * u;
                    update4<RULE, SCALED, DECAY>(P[u], G[u], A[u], B[u], r.a, r.b, gs, r.d, k);
                    p4[i] = P[u];
                    s14[i] = A[u];
                    if constexpr (RULE == kAdam) s24[i] = B[u];
                }
            } else {
                const int cnt4 = cnt >> 2;
                for (int i = tid; i < cnt4; i += 256) {
                    const float4 G = g4[i];
                    float4 P = p4[i], A = s14[i];
                    float4 B = RULE == kAdam ? s24[i] : make_float4(0.f, 0.f, 0.f, 0.f);
                    update4<RULE, SCALED, DECAY>(P, G, A, B, r.a, r.b, gs, r.d, k);
                    p4[i] = P;
                    s14[i] = A;
                    if constexpr (RULE == kAdam) s24[i] = B;
                }
                const int i = 4 * cnt4 + tid;       // the tail of 1-3 elements
                if (i < cnt) {
                    float P = p[i], A = s1[i], B = RULE == kAdam ? s2[i] : 0.f;
                    update1<RULE, SCALED, DECAY>(P, g[i], A, B, r.a, r.b, gs, r.d, k);
                    p[i] = P;
                    s1[i] = A;
                    if constexpr (RULE == kAdam) s2[i] = B;
                }
            }
        } else {
            for (int i = tid; i < cnt; i += 256) {
                float P = p[i], A = s1[i], B = RULE == kAdam ? s2[i] : 0.f;
                update1<RULE, SCALED, DECAY>(P, g[i], A, B, r.a, r.b, gs, r.d, k);
                p[i] = P;
                s1[i] = A;
                if constexpr (RULE == kAdam) s2[i] = B;
            }
        }
    }
}

bool finite_nonneg(double x) { return isfinite(x) && x >= 0.0; }

double decay_of(const aspire_optim_tensor&) { return 0.0; }
double decay_of(const aspire_adamw_tensor& t) { return t.weight_decay; }

template <int RULE, bool SCALED, bool DECAY>
void launch_step(unsigned grid, hipStream_t st, const OptimRec* recs, const int32_t* prefix, int n_tensors, int chunks, const OptimCoef& k,
                 const float* grad_scale) {
    hipLaunchKernelGGL((optim_step_kernel<RULE, SCALED, DECAY>), dim3(grid), dim3(256), 0, st, recs, prefix, n_tensors, chunks, k, grad_scale);
}

// T: aspire_optim_tensor (no decay), aspire_adamw_tensor (decoupled decay, Adam's rule); grad_scale NULL: the unscaled kernel
template <class T>
int optim_step(int rule, const char* who, const T* tensors, int64_t n_tensors, double beta1, double beta2, double eps, double lr_decay,
               const float* grad_scale, void* ws, size_t ws_bytes, void* stream) {
    constexpr bool kDecay = std::is_same<T, aspire_adamw_tensor>::value;
    ASPIRE_REQUIRE(((uintptr_t)grad_scale & 3) == 0, ASPIRE_ERR_INVALID_ARG, "%s: grad_scale is not 4-byte aligned", who);
    ASPIRE_REQUIRE(n_tensors >= 0, ASPIRE_ERR_INVALID_ARG, "%s: n_tensors = %lld is negative", who, (long long)n_tensors);
    ASPIRE_REQUIRE(finite_nonneg(eps), ASPIRE_ERR_INVALID_ARG, "%s: eps = %g must be finite and >= 0", who, eps);
    if (rule == kAdam) {
        ASPIRE_REQUIRE(beta1 >= 0.0 && beta1 < 1.0, ASPIRE_ERR_INVALID_ARG, "%s: beta1 = %g outside [0, 1)", who, beta1);
        ASPIRE_REQUIRE(beta2 >= 0.0 && beta2 < 1.0, ASPIRE_ERR_INVALID_ARG, "%s: beta2 = %g outside [0, 1)", who, beta2);
    } else {
        ASPIRE_REQUIRE(finite_nonneg(lr_decay), ASPIRE_ERR_INVALID_ARG, "%s: lr_decay = %g must be finite and >= 0", who, lr_decay);
    }
    if (n_tensors == 0) return ASPIRE_OK;
    ASPIRE_REQUIRE(tensors, ASPIRE_ERR_INVALID_ARG, "%s: null tensor table with n_tensors = %lld", who, (long long)n_tensors);
    int64_t chunks = 0;
    for (int64_t i = 0; i < n_tensors; ++i) {
        const T& t = tensors[i];
        ASPIRE_REQUIRE(t.n >= 0, ASPIRE_ERR_INVALID_ARG, "%s: tensor %lld has n = %lld", who, (long long)i, (long long)t.n);
        ASPIRE_REQUIRE(t.step >= 1, ASPIRE_ERR_INVALID_ARG, "%s: tensor %lld has step = %lld (the first step is 1)", who, (long long)i,
                       (long long)t.step);
        ASPIRE_REQUIRE(finite_nonneg(t.lr), ASPIRE_ERR_INVALID_ARG, "%s: tensor %lld has lr = %g (must be finite and >= 0)", who,
                       (long long)i, t.lr);
        ASPIRE_REQUIRE(finite_nonneg(decay_of(t)), ASPIRE_ERR_INVALID_ARG, "%s: tensor %lld has weight_decay = %g (must be finite and >= 0)",
                       who, (long long)i, decay_of(t));
        ASPIRE_REQUIRE(t.n == 0 || (t.param && t.grad && t.state1 && (rule == kAdagrad || t.state2)), ASPIRE_ERR_INVALID_ARG,
                       "%s: tensor %lld has a null param / grad / state pointer with n = %lld", who, (long long)i, (long long)t.n);
        ASPIRE_REQUIRE((((uintptr_t)t.param | (uintptr_t)t.grad | (uintptr_t)t.state1 | (rule == kAdam ? (uintptr_t)t.state2 : 0)) & 3) == 0,
                       ASPIRE_ERR_INVALID_ARG, "%s: tensor %lld has a pointer that is not 4-byte aligned", who, (long long)i);
        chunks += chunks_of(t.n);
        ASPIRE_REQUIRE(chunks < ((int64_t)1 << 31), ASPIRE_ERR_UNSUPPORTED, "%s: more than 2^31 chunks of %d elements", who, kOptimChunk);
    }
    const size_t need = table_bytes(n_tensors);
    ASPIRE_REQUIRE(ws, ASPIRE_ERR_INVALID_ARG, "%s: null workspace (aspire_optim_workspace_bytes(%lld) = %zu)", who, (long long)n_tensors,
                   need);
    ASPIRE_REQUIRE(ws_bytes >= need, ASPIRE_ERR_INVALID_ARG, "%s: workspace of %zu bytes is too small, need %zu", who, ws_bytes, need);
    ASPIRE_REQUIRE(((uintptr_t)ws & 15) == 0, ASPIRE_ERR_INVALID_ARG, "%s: workspace is not 16-byte aligned", who);
    if (chunks == 0) return ASPIRE_OK;

    hipStream_t st = static_cast<hipStream_t>(stream);
    Staging staging;        // (multi_tensor.h: the pinned ring shared with the gradient bucket)
    if (const int rc = staging.acquire(who, need)) return rc;

    OptimRec* recs = static_cast<OptimRec*>(staging.host());
    int32_t* prefix = reinterpret_cast<int32_t*>(recs + n_tensors);
    int32_t at = 0;
    for (int64_t i = 0; i < n_tensors; ++i) {
        const T& t = tensors[i];
        OptimRec r = {};
        r.p = t.param;
        r.g = t.grad;
        r.s1 = t.state1;
        r.s2 = rule == kAdam ? t.state2 : nullptr;
        r.n = t.n;
        if (rule == kAdam) {
            // torch/optim/adam.py _single_tensor_adam: python floats, i.e. doubles
            const double bc1 = 1.0 - pow(beta1, (double)t.step), bc2 = 1.0 - pow(beta2, (double)t.step);
            r.a = (float)(t.lr / bc1);
            r.b = (float)sqrt(bc2);
        } else {
            r.a = (float)(t.lr / (1.0 + (double)(t.step - 1) * lr_decay));
        }
        // torch/optim/adam.py, decoupled_weight_decay: param.mul_(1 - lr * weight_decay), the factor a python float
        r.d = (float)(1.0 - t.lr * decay_of(t));
        r.vec = (((uintptr_t)t.param | (uintptr_t)t.grad | (uintptr_t)t.state1 | (uintptr_t)r.s2) & 15) == 0;
        recs[i] = r;
        prefix[i] = at;
        at += (int32_t)chunks_of(t.n);
    }
    prefix[n_tensors] = at;
    if (const int rc = staging.commit(ws, st)) return rc;

    const OptimRec* d_recs = static_cast<const OptimRec*>(ws);
    const int32_t* d_prefix = reinterpret_cast<const int32_t*>(d_recs + n_tensors);
    const OptimCoef k = {(float)(1.0 - beta1), (float)beta2, (float)(1.0 - beta2), (float)eps};
    const unsigned grid = (unsigned)(at < kOptimMaxGrid ? at : kOptimMaxGrid);
    const int nt = (int)n_tensors, nc = (int)at;
    if constexpr (kDecay) {
        if (grad_scale) launch_step<kAdam, true, true>(grid, st, d_recs, d_prefix, nt, nc, k, grad_scale);
        else launch_step<kAdam, false, true>(grid, st, d_recs, d_prefix, nt, nc, k, grad_scale);
    } else if (rule == kAdam) {
        if (grad_scale) launch_step<kAdam, true, false>(grid, st, d_recs, d_prefix, nt, nc, k, grad_scale);
        else launch_step<kAdam, false, false>(grid, st, d_recs, d_prefix, nt, nc, k, grad_scale);
    } else {
        if (grad_scale) launch_step<kAdagrad, true, false>(grid, st, d_recs, d_prefix, nt, nc, k, grad_scale);
        else launch_step<kAdagrad, false, false>(grid, st, d_recs, d_prefix, nt, nc, k, grad_scale);
    }
    ASPIRE_LAUNCH_OK();
    return ASPIRE_OK;
}

}  // namespace
}  // namespace aspire

extern "C" size_t aspire_optim_workspace_bytes(int64_t n_tensors) { return n_tensors > 0 ? aspire::table_bytes(n_tensors) : 16; }

extern "C" int aspire_adam_step_f32(const aspire_optim_tensor* tensors, int64_t n_tensors, double beta1, double beta2, double eps,
                                    void* workspace, size_t workspace_bytes, void* stream) {
    return aspire::optim_step(aspire::kAdam, "aspire_adam_step_f32", tensors, n_tensors, beta1, beta2, eps, 0.0, nullptr, workspace,
                              workspace_bytes, stream);
}

extern "C" int aspire_adagrad_step_f32(const aspire_optim_tensor* tensors, int64_t n_tensors, double lr_decay, double eps, void* workspace,
                                       size_t workspace_bytes, void* stream) {
    return aspire::optim_step(aspire::kAdagrad, "aspire_adagrad_step_f32", tensors, n_tensors, 0.0, 0.0, eps, lr_decay, nullptr, workspace,
                              workspace_bytes, stream);
}

// The same steps on gradients times *grad_scale (a device float, aspire_grad_norm_f32's out + 1): NULL gives the kernels above.
extern "C" int aspire_adam_step_scaled_f32(const aspire_optim_tensor* tensors, int64_t n_tensors, double beta1, double beta2, double eps,
                                           const float* grad_scale, void* workspace, size_t workspace_bytes, void* stream) {
    return aspire::optim_step(aspire::kAdam, "aspire_adam_step_scaled_f32", tensors, n_tensors, beta1, beta2, eps, 0.0, grad_scale, workspace,
                              workspace_bytes, stream);
}

extern "C" int aspire_adagrad_step_scaled_f32(const aspire_optim_tensor* tensors, int64_t n_tensors, double lr_decay, double eps,
                                              const float* grad_scale, void* workspace, size_t workspace_bytes, void* stream) {
    return aspire::optim_step(aspire::kAdagrad, "aspire_adagrad_step_scaled_f32", tensors, n_tensors, 0.0, 0.0, eps, lr_decay, grad_scale,
                              workspace, workspace_bytes, stream);
}

extern "C" int aspire_adamw_step_f32(const aspire_adamw_tensor* tensors, int64_t n_tensors, double beta1, double beta2, double eps,
                                     const float* grad_scale, void* workspace, size_t workspace_bytes, void* stream) {
    return aspire::optim_step(aspire::kAdam, "aspire_adamw_step_f32", tensors, n_tensors, beta1, beta2, eps, 0.0, grad_scale, workspace,
                              workspace_bytes, stream);
}
