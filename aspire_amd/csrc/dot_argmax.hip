// Where a pair's largest sentence dot product sits: the alignment step of the co-citation data path (include/aspire_hip.h, A16).
//
//   arg[p] = (i, j) = np.unravel_index(np.matmul(q, c.T).argmax(), (q_len, c_len)),  best[p] = <q_i, c_j>
//   (pre_proc_cocits.py:487-494: three such calls per training example).
//
// dotmax_pair_kernel's frame and arithmetic (pair_fwd.h: one wave per PAIRED pair, 16 x 16 tiles over documents of up to 128 rows;
// dot_tiles.h: mfma8 into four accumulators, (acc0 + acc1) + (acc2 + acc3)), so best[p] has the bits aspire_dotmax_scores_f32 gives the
// pair with ASPIRE_SIM_DOT.  The tile walk meets the entries candidate tiles outer, query tiles inner, spread over lanes and registers,
// while numpy's pick is defined in row-major order of [q_len, c_len]: every entry gets a 64-bit key whose order IS numpy's rule, and
// the pick is the largest key whatever the order of the visits --
//   high half  the order-preserving image of the float's bits (sign bit set for x >= 0, all bits flipped for x < 0), -0.0 taken as
//              +0.0 (they tie), a NaN as 0xFFFFFFFF, above +inf (np.argmax takes a NaN for the maximum)
//   low half   0xFFFFFFFF - (i * c_len + j): of equal values the first in row-major order wins -- the first NaN, and (0, 0) in a
//              block of all -inf, whose keys are still above an entry's that does not exist (0)
// A lane keeps its largest key and that entry's value; one 64-bit max over the wave; the lane that owns the winner (keys are
// distinct) writes arg and best.  No atomics: every output has one writer, every run the same bits.
//   poison     a document longer than its set's host bound: arg = (-1, -1), best = NaN (pair_fwd.h's rule)
//   empty      a pair with a document of no rows: arg = (-1, -1), best = -inf (the host layer raises before, as numpy does)
#include <math.h>

#include "common.h"
#include "pair_fwd.h"

namespace aspire {
namespace {

struct ArgmaxArgs : PairArgs {      // scores: best [P], or null
    int32_t* arg;                   // [P, 2]
};

__device__ __forceinline__ uint64_t pick_key(float x, int e) {
    const uint32_t u = __float_as_uint(x);
    uint32_t hi = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    if (x == 0.0f) hi = 0x80000000u;
    if (x != x) hi = 0xFFFFFFFFu;
    return ((uint64_t)hi << 32) | (0xFFFFFFFFu - (uint32_t)e);
}

__device__ __forceinline__ uint64_t wave_max_key(uint64_t k) {
#pragma unroll
    for (int sh = 1; sh < 64; sh <<= 1) {
        const uint64_t o = __shfl_xor((unsigned long long)k, sh);
        k = o > k ? o : k;
    }
    return k;
}

__device__ __forceinline__ void write_pick(const ArgmaxArgs& a, int64_t p, int i, int j, float best) {
    a.arg[2 * p] = i;
    a.arg[2 * p + 1] = j;
    if (a.scores) a.scores[p] = best;
}

__global__ void __launch_bounds__(256) dot_argmax_pair_kernel(ArgmaxArgs a, int64_t P) {
    const int64_t p = wave_pair();
    if (p >= P) return;
    const PairWave w = pair_wave(a.q, a.c, kModePaired, nullptr, 0, p);
    if (w.poison || w.ql <= 0 || w.cl <= 0) {
        if (w.lane == 0) write_pick(a, p, -1, -1, w.poison ? __builtin_nanf("") : -INFINITY);
        return;
    }
    uint64_t key = 0;
    float val = -INFINITY;
    const float *qbase = w.qdoc + 8 * w.g, *cbase = w.cdoc + 8 * w.g;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    for (int c0 = 0; c0 < w.cl; c0 += 16) {
        const bool va = tile_row_valid(w.r, c0, w.cl);
        const float* pa = tile_row(w.r, cbase, c0, w.cl);
        for (int q0 = 0; q0 < w.ql; q0 += 16) {
            const bool vb = tile_row_valid(w.r, q0, w.ql);
            const float* pb = tile_row(w.r, qbase, q0, w.ql);
            f32x4 acc[4] = {zero, zero, zero, zero};
            for (int s = 0; s < kD / 32; ++s) {
                const f32x4 a0 = va ? ld4(pa + 32 * s) : zero, a1 = va ? ld4(pa + 32 * s + 4) : zero;
                const f32x4 b0 = vb ? ld4(pb + 32 * s) : zero, b1 = vb ? ld4(pb + 32 * s + 4) : zero;
                mfma8(a0, a1, b0, b1, acc);
            }
            const f32x4 dot = (acc[0] + acc[1]) + (acc[2] + acc[3]);
            const int e0 = (q0 + w.r) * w.cl + c0 + 4 * w.g;       // this lane's query row against candidate row c0 + 4 g
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                if (!entry_valid(w, c0, v, vb)) continue;
                const uint64_t k = pick_key(dot[v], e0 + v);
                if (k > key) {
                    key = k;
                    val = dot[v];
                }
            }
        }
    }
    const uint64_t win = wave_max_key(key);
    if (key == win) {       // one lane: a valid entry's key is above 0 and no two entries share one
        const int e = (int)(0xFFFFFFFFu - (uint32_t)win);
        const int i = e / w.cl;
        write_pick(a, p, i, e - i * w.cl, val);
    }
}

}  // namespace
}  // namespace aspire

using namespace aspire;

extern "C" int aspire_dot_argmax_f32(const aspire_repset* q, const aspire_repset* c, int64_t D, int32_t* arg, float* best,
                                     void* stream) {
    if (int rc = check_dot_sets(q, c, D, ASPIRE_PAIR_PAIRED, ASPIRE_SIM_DOT)) return rc;
    if (q->n == 0) return ASPIRE_OK;
    ASPIRE_REQUIRE(arg, ASPIRE_ERR_INVALID_ARG, "arg is null");
    const ArgmaxArgs a{pair_args(q, c, ASPIRE_PAIR_PAIRED, best), arg};
    return launch_pair_waves(dot_argmax_pair_kernel, a, q->n, (hipStream_t)stream);
}
