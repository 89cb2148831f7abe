// The frame the forward kernels of the sentence-pair dot-product scores share (dotmax.hip, jointsm.hip, l2agg_pair.hip), apart from
// each score's own tile epilogue.  dot_tiles.h keeps the operand and product helpers; this header holds who works on what.
//
// One wave per pair (dotmax_pair_kernel, jointsm_pair_kernel, l2agg_pair_kernel): four pairs per workgroup of 256 threads, pair
// p = 4 blockIdx.x + wave (the last workgroup's waves beyond P leave at once), 16 x 16 tiles over documents of up to 128 rows.
//   index     CROSS p = qi C + ci, PAIRED qi = ci = p, MAPPED ci = p and qi = the job of candidate p (job_of: empty jobs skipped)
//   poison    a document longer than its set's host-known bound: the score is NaN; the kernel leaves itself (jointsm fills a block)
//   tiles     lane l holds candidate row c0 + (l & 15) as the A operand and query row q0 + (l & 15) as the B operand, the k values
//             8 (l >> 4) + 32 s + e of both; a lane whose row lies beyond the document reads row 0's address and loads nothing.
//             Accumulator register v of lane l is C[candidate row c0 + 4 (l >> 4) + v][query row q0 + (l & 15)] (entry_valid).
// CROSS with documents of <= 16 rows (dotmax_cross_kernel, jointsm_cross_kernel): a workgroup stages 32 candidate row slots
// (documents padded to a power of two W_c <= 16) in LDS and its four waves stream the query rows in chunks of 16 slots; one
// document pair's entries of a tile sit on W_q neighbouring lanes x W_c rows.  The host side: one launcher for each of the two.
#pragma once
#include <math.h>

#include "common.h"
#include "dot_tiles.h"

namespace aspire {
namespace {

// what the kernels' argument structs share (DotArgs, JsmArgs, L2aggArgs derive from it)
struct PairArgs {
    DotSet q, c;
    int mode;
    const int32_t* job_off;     // kModeMapped: [J + 1]
    int32_t J;
    int32_t wq_log, wc_log;     // cross kernels: log2 of the row slots per document
    float* scores;
};

// ---- one wave per pair ---------------------------------------------------------------------------------------------------
__device__ __forceinline__ int64_t wave_pair() { return (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); }

struct PairWave {
    int lane, g, r;                 // lane, its k group l >> 4 and its row l & 15
    int ql, cl;                     // the documents' rows
    const float *qdoc, *cdoc;       // their first rows
    bool poison;                    // longer than the host-known bound
};
__device__ __forceinline__ PairWave pair_wave(const DotSet& q, const DotSet& c, int mode, const int32_t* job_off, int32_t J, int64_t p) {
    PairWave w;
    w.lane = threadIdx.x & 63;
    w.g = w.lane >> 4;
    w.r = w.lane & 15;
    int64_t qi, ci;
    if (mode == kModeCross) {
        qi = p / c.n;
        ci = p - qi * c.n;
    } else if (mode == kModePaired) {
        qi = ci = p;
    } else {
        ci = p;
        qi = job_of(job_off, J, p);
    }
    w.ql = q.len[qi];
    w.cl = c.len[ci];
    w.poison = w.ql > q.bound || w.cl > c.bound;
    w.qdoc = q.rows + (int64_t)q.start[qi] * kD;
    w.cdoc = c.rows + (int64_t)c.start[ci] * kD;
    return w;
}
__device__ __forceinline__ void poison_score(float* scores, int64_t p, int lane) { if (lane == 0) scores[p] = __builtin_nanf(""); }

// Lane row r's operand row of the tile that starts at row0 of a document (`base` = its first row + the lane's 8 g): does the
// document have it, and its address -- row 0's for a masked lane, which loads nothing.  (r as the kernel's own int, and the compare
// asked again instead of passed as a bool: NOTES.md, "The pair forward kernels' shared frame", on jointsm_pair_kernel's registers.)
__device__ __forceinline__ bool tile_row_valid(int r, int row0, int len) { return row0 + r < len; }
__device__ __forceinline__ const float* tile_row(int r, const float* base, int row0, int len) {
    return base + (int64_t)(row0 + r < len ? row0 + r : 0) * kD;
}
// accumulator register v of this lane: candidate row c0 + 4 g + v against the lane's query row (vb: the document has it)
__device__ __forceinline__ bool entry_valid(const PairWave& w, int c0, int v, bool vb) { return c0 + 4 * w.g + v < w.cl && vb; }

// the four lanes that share l & 15 hold the partial sums of one row: the same bits in all four
__device__ __forceinline__ float rowgroup_sum(float v) {
    v += lane_xor<16>(v);
    return v + lane_xor<32>(v);
}

// The soft-max of a pair's block, shifted by the running maximum m of its entries x: beside S = sum e with e = ex(x - m), the CENTRED
// T = sum e (x - m), so that sum p x = m + T / S (jointsm.hip's header).  raise(tile_max) is wave-uniform (one wave_max per tile) and
// comes before the tile's add(x); a new maximum m' rescales with f = ex(m - m'): S <- f S, T <- f (T + (m - m') S).  S and T stay per
// lane: the caller ends with wave_sum of both.  ex(y), y <= 0, is the kernel's own exponential of the scaled difference.
struct CentredSoftmax {
    float m = -INFINITY, S = 0.f, T = 0.f;
    template <class Exp>
    __device__ __forceinline__ void raise(float tile_max, Exp ex) {
        if (tile_max > m) {
            if (m > -INFINITY) {
                const float dm = m - tile_max, f = ex(dm);
                T = f * fmaf(dm, S, T);
                S = f * S;
            }
            m = tile_max;
        }
    }
    template <class Exp>
    __device__ __forceinline__ void add(float x, Exp ex) {
        const float y = x - m, e = ex(y);
        S += e;
        T = fmaf(e, y, T);
    }
};

// ---- CROSS, documents of <= 16 rows: 32 candidate row slots per workgroup in LDS --------------------------------------
// row slot vrow of a set whose documents take 1 << w_log slots each: its document, and whether the slot holds one of its rows
struct Slot {
    int64_t doc;
    int row;
    bool valid;
};
__device__ __forceinline__ Slot slot_of(const DotSet& set, int w_log, int64_t vrow) {
    Slot s;
    s.doc = vrow >> w_log;
    s.row = (int)(vrow & ((1 << w_log) - 1));
    s.valid = s.doc < set.n && s.row < set.len[s.doc < set.n ? s.doc : 0];
    return s;
}

// Stage the workgroup's slots slot0 .. slot0 + 31 into As, zeros where a slot holds no row: four threads per slot (waves 0 and 1),
// thread gs reads k = 32 s + 8 gs .. + 7 -- the k values lane group gs of the pair kernels reads, so a pair's dot products have the
// same bits in both forms.  NORMS: a slot's sum of squares into nrm_c, summed as the pair kernel sums it.  The caller's barrier follows.
template <bool NORMS>
__device__ __forceinline__ void stage_slots(const DotSet& c, int wc_log, int64_t slot0, float* As, float* nrm_c) {
    const int tid = threadIdx.x;
    if (tid >= 4 * kXRows) return;
    const int R = tid >> 2, gs = tid & 3;
    const Slot sl = slot_of(c, wc_log, slot0 + R);
    const float* src = sl.valid ? c.rows + ((int64_t)c.start[sl.doc] + sl.row) * kD + 8 * gs : nullptr;
    float* dst = As + R * kXStride + 8 * gs;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    float ss = 0.f;
#pragma unroll 4
    for (int s = 0; s < kD / 32; ++s) {
        const f32x4 x0 = sl.valid ? ld4(src + 32 * s) : zero, x1 = sl.valid ? ld4(src + 32 * s + 4) : zero;
        if constexpr (NORMS) ss = sumsq8(ss, x0, x1);
        *reinterpret_cast<f32x4*>(dst + 32 * s) = x0;
        *reinterpret_cast<f32x4*>(dst + 32 * s + 4) = x1;
    }
    if constexpr (NORMS) {
        ss += lane_xor<1>(ss);             // (g0 + g1) + (g2 + g3), as rowgroup_sum
        ss += lane_xor<2>(ss);
        if (gs == 0) nrm_c[R] = ss;
    }
}

// a wave's chunk qc of 16 query row slots: the lane's slot, its document's length (0 beyond Q) and its operand address
struct QueryChunk {
    int64_t qdoc;
    int qlen;
    bool vb;
    const float* pb;
};
__device__ __forceinline__ QueryChunk query_chunk(const DotSet& q, int wq_log, int64_t qc, int g, int r) {
    QueryChunk k;
    const int64_t vq = qc * 16 + r;
    k.qdoc = vq >> wq_log;
    const int qrow = (int)(vq & ((1 << wq_log) - 1));
    k.qlen = k.qdoc < q.n ? q.len[k.qdoc] : 0;
    k.vb = qrow < k.qlen;
    k.pb = q.rows + (k.vb ? ((int64_t)q.start[k.qdoc] + qrow) * kD : 0) + 8 * g;
    return k;
}

// all-reduce over one document pair's entries of a 16 x 16 tile: the query document's rows sit on Wq neighbouring lanes, the
// candidate document's Wc rows on registers v, then lane groups g
template <typename Op>
__device__ __forceinline__ void pair_block_allreduce(float (&m)[4], int Wq, int Wc, Op op) {
#pragma unroll
    for (int v = 0; v < 4; ++v)
        for (int sh = 1; sh < Wq; sh <<= 1) m[v] = op(m[v], __shfl_xor(m[v], sh));
    if (Wc >= 2) {
        m[0] = m[1] = op(m[0], m[1]);
        m[2] = m[3] = op(m[2], m[3]);
    }
    if (Wc >= 4) m[0] = m[1] = m[2] = m[3] = op(m[0], m[2]);
    if (Wc >= 8) {
        m[0] = op(m[0], __shfl_xor(m[0], 16));
        if (Wc >= 16) m[0] = op(m[0], __shfl_xor(m[0], 32));
        m[1] = m[2] = m[3] = m[0];
    }
}

// The writers of tile t (candidate slots slot0 + 16 t ..): of a document pair's Wq lanes x Wc rows the first lane, lane group and
// register store score(v); NaN where a document is longer than its bound (the bound, not its row slots).
template <class Score>
__device__ __forceinline__ void write_pair_scores(const PairArgs& a, int64_t slot0, int t, int g, int r, const QueryChunk& k, Score score) {
    const DotSet &q = a.q, &c = a.c;
    const int Wc = 1 << a.wc_log, Wq = 1 << a.wq_log;
    const int vstep = Wc < 4 ? Wc : 4;
    const bool g_writes = Wc < 8 || (g & (Wc / 4 - 1)) == 0;
    if ((r & (Wq - 1)) == 0 && k.qdoc < q.n && g_writes) {
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            if (v % vstep) continue;
            const int64_t cdoc = (slot0 + 16 * t + 4 * g + v) >> a.wc_log;
            if (cdoc >= c.n) continue;
            const bool too_long = k.qlen > q.bound || c.len[cdoc] > c.bound;
            a.scores[k.qdoc * c.n + cdoc] = too_long ? __builtin_nanf("") : score(v);
        }
    }
}

// ---- host ----------------------------------------------------------------------------------------------------------------
// one wave per pair, four pairs per workgroup: kernel(args, P)
template <class Args>
int launch_pair_waves(void (*kernel)(Args, int64_t), const Args& args, int64_t P, hipStream_t stream) {
    const int64_t blocks = (P + 3) / 4;
    ASPIRE_REQUIRE(blocks < ((int64_t)1 << 31), ASPIRE_ERR_UNSUPPORTED, "too many pairs: %lld", (long long)P);
    hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(256), 0, stream, args, P);
    ASPIRE_LAUNCH_OK();
    return ASPIRE_OK;
}

// CROSS with documents of <= 16 rows on both sides takes the cross kernel: kernel(args), the row slots per document filled in here
inline bool cross_form(const PairArgs& a) { return a.q.bound <= 16 && a.c.bound <= 16; }
inline int log2_slots(int rows) {
    int l = 0;
    while ((1 << l) < rows) ++l;
    return l;
}
template <class Args>
int launch_cross_slots(void (*kernel)(Args), Args& a, hipStream_t stream) {
    a.mode = kModeCross;
    a.wq_log = log2_slots(a.q.bound);
    a.wc_log = log2_slots(a.c.bound);
    const int64_t blocks = ((a.c.n << a.wc_log) + kXRows - 1) / kXRows;
    ASPIRE_REQUIRE(blocks < ((int64_t)1 << 31), ASPIRE_ERR_UNSUPPORTED, "too many candidates: %lld", (long long)a.c.n);
    hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(256), 0, stream, a);
    ASPIRE_LAUNCH_OK();
    return ASPIRE_OK;
}

// the shared arguments of a call: CROSS / PAIRED by `pairing`, or the batched entries' jobs
inline PairArgs pair_args(const aspire_repset* q, const aspire_repset* c, int pairing, float* scores) {
    return PairArgs{to_dot(q), to_dot(c), pairing == ASPIRE_PAIR_CROSS ? kModeCross : kModePaired, nullptr, 0, 0, 0, scores};
}
inline PairArgs mapped_pair_args(const aspire_repset* q, const aspire_repset* c, const int32_t* job_off, float* scores) {
    return PairArgs{to_dot(q), to_dot(c), kModeMapped, job_off, (int32_t)q->n, 0, 0, scores};
}

}  // namespace
}  // namespace aspire
