// VALU tiles for documents of up to 32 sentence rows: masked pairwise L2 (A5) into the otAspire workspace slots, max-sim and
// its sibling aggregations (A9), the per-query boxes, the long-pair census, the batch bounding-box diameter.  Reference arithmetic:
//   src/learning/facetid_models/pair_distances.py:21-60, :138-186 (allenai/aspire); geomloss==0.2.4 squared_distances (restated).
//
// Data layout and work decomposition (gfx950, wave = 64 lanes):
//   * one workgroup = 3 waves = one candidate document x a chunk of queries.  Wave w owns encoding
//     coordinates [256w, 256w+256): lane l holds the float4 at d = 256w + 4l of every sentence row, so a
//     768-float row is ONE global_load_dwordx4 per lane, perfectly coalesced, no LDS staging.
//   * sentence-pair sums are formed 8x8 rows at a time ("tile"): each lane accumulates the 64
//     (i,j) partial sums over its 4 coordinates, then a 63-exchange halving butterfly
//     (v_permlane32_swap / v_permlane16_swap / DPP) leaves lane l = 8*i + j holding the wave's sum for
//     (i,j).  The three waves' partials meet in LDS (6 KB per tile).
//
// Host side (the end of the file): one launcher per kernel, declared in score_types.h.  launch_cost_stage picks among the cost
// forms of one chunk of candidates; which call takes the cost stage at all is score.hip's business.
#include <math.h>

#include "common.h"
#include "tuning.h"
#include "forms.h"
#include "score_types.h"
#include "score_device.h"
#include "exact_d2.h"

namespace aspire {
namespace {

// LDS carve (floats): red[kWaves][T*T][128] | rednorm[kWaves][T][16] | reddiam[4] | redo_mask (8 B) + pad | xpose[kWaves][32][68]
constexpr int kXpLd = 68;                 // row stride of the transpose scratch: 64 lanes + 4 (keeps b128 reads
constexpr int kXpWave = 32 * kXpLd;       // 16 B aligned and spreads the 16-lane read groups over all bank slots)
template <int T>
struct Lds {
    static constexpr int kRed = kWaves * T * T * 128;
    static constexpr int kNorm = kWaves * T * 16;
    static constexpr int kRedo = kRed + kNorm + 4;   // 64-bit mask of entries to redo (pair_cost1_body): a word no reduction scratch touches
    static constexpr int kXp = kRedo + 4;
    static constexpr int kTotal = kXp + kWaves * kXpWave;
};

// Sum N per-lane partials across the 64 lanes of a wave through LDS instead of cross-lane VALU ops: every lane
// stores its N values as a column (conflict-free ds_write_b32), then lane l reads back 64*N/64... = a contiguous
// piece of row (l * N / 64) as b128s and adds it up.  Element e ends up in the 64/N lanes e*64/N ...; returns it.
// On gfx950 a v_permlane*_swap costs ~22 issue cycles and a DPP op ~8 (build/dbg/thr.hip), so the 31-exchange
// register butterfly this replaces was 4x the cost of the 768 multiply-adds it served.
template <int N>
__device__ __forceinline__ float lds_wave_reduce(const float (&v)[N], float* xp, int lane) {
    static_assert(N == 32 || N == 16, "sizes used here");
#pragma unroll
    for (int k = 0; k < N; ++k) xp[k * kXpLd + lane] = v[k];
    // DS operations of one wave execute in order: the loads below see the stores above (other waves use
    // their own scratch).  The fence only stops the compiler from reordering them.
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    constexpr int kLanesPer = 64 / N;         // lanes sharing one element
    constexpr int kFloats = 64 / kLanesPer;   // floats each of them adds up
    const float4* row = reinterpret_cast<const float4*>(xp + (lane / kLanesPer) * kXpLd + (lane % kLanesPer) * kFloats);
    float s = 0.f;
#pragma unroll
    for (int m = 0; m < kFloats / 4; ++m) {
        const float4 t = row[m];
        s += (t.x + t.y) + (t.z + t.w);
    }
    s += lane_xor<1>(s);
    if constexpr (kLanesPer == 4) s += lane_xor<2>(s);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");   // the scratch is rewritten by the next call
    __builtin_amdgcn_wave_barrier();
    return s;
}

// Load N sentence rows (this lane's float4 slice) of one document; rows >= navail read as zero.
template <int N, bool BBOX, bool CENTER = false>
__device__ __forceinline__ void load_rows(float4 (&r)[N], const float* doc, int row0, int navail, int dofs, int nbox,
                                          float4& mn, float4& mx, const float4& mu) {
#pragma unroll
    for (int i = 0; i < N; ++i) {
        const int row = row0 + i;
        r[i] = row < navail ? ld4(doc + (size_t)row * kD + dofs) : make_float4(0.f, 0.f, 0.f, 0.f);
        if constexpr (CENTER)                 // ASPIRE_OT_FLAG_CENTER (a row past the document stays a zero row: masked downstream)
            if (row < navail) { r[i].x -= mu.x; r[i].y -= mu.y; r[i].z -= mu.z; r[i].w -= mu.w; }
        if (BBOX && row < nbox) {
            mn.x = fminf(mn.x, r[i].x); mn.y = fminf(mn.y, r[i].y); mn.z = fminf(mn.z, r[i].z); mn.w = fminf(mn.w, r[i].w);
            mx.x = fmaxf(mx.x, r[i].x); mx.y = fmaxf(mx.y, r[i].y); mx.z = fmaxf(mx.z, r[i].z); mx.w = fmaxf(mx.w, r[i].w);
        }
    }
}

// Per-wave partial sums of half an 8x8 tile (4 query rows x 8 candidate rows) -> LDS.
// red layout: [tile][2][64] (0: x.y dot, 1: sum (x-y)^2), element 8*i + j.  Only 32 accumulators, 4 query
// rows and 8 candidate rows are live at a time (64 accumulators + both 8-row operand tiles cap the kernel
// at 2 waves/SIMD and a 1000-block grid then runs in two rounds).  lds_wave_reduce leaves element e in lanes
// 2e and 2e+1; even lanes write it.
template <bool NEED_G, bool NEED_D2>
__device__ __forceinline__ void half_tile_partials(const float4 (&x)[4], const float4 (&y)[8], float* red_half,
                                                   float* xp, int lane) {
    if constexpr (NEED_D2) {
        float acc[32];
#pragma unroll
        for (int j = 0; j < 8; ++j)      // candidate row outer: row j is needed only when its load has landed
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float dx = x[i].x - y[j].x, dy = x[i].y - y[j].y, dz = x[i].z - y[j].z, dw = x[i].w - y[j].w;
                acc[i * 8 + j] = fmaf(dw, dw, fmaf(dz, dz, fmaf(dy, dy, dx * dx)));
            }
        const float r = lds_wave_reduce<32>(acc, xp, lane);
        if ((lane & 1) == 0) red_half[64 + (lane >> 1)] = r;
    }
    __builtin_amdgcn_sched_barrier(0);  // do not overlap the passes: that doubles the live accumulators
    if constexpr (NEED_G) {
        float acc[32];
#pragma unroll
        for (int j = 0; j < 8; ++j)
#pragma unroll
            for (int i = 0; i < 4; ++i)
                acc[i * 8 + j] = dot4(x[i], y[j]);
        const float r = lds_wave_reduce<32>(acc, xp, lane);
        if ((lane & 1) == 0) red_half[(lane >> 1)] = r;
    }
    __builtin_amdgcn_sched_barrier(0);
}

// ---------------------------------------------------------------------------------------------
// Phase 1: all three waves form the partial sums of (query doc, candidate doc) for every tile.
// ---------------------------------------------------------------------------------------------
template <int T, bool NEED_G, bool NEED_D2, bool BBOX, bool CENTER = false>
__device__ __forceinline__ void pair_partials(const float* qdoc, int q_avail, int q_box, const float* cdoc, int c_avail,
                                              int c_box, float* lds, int wave, int lane) {
    const int dofs = wave * 256 + lane * 4;
    // CENTER -- rows sharing a large common component (include/aspire_hip.h: ASPIRE_OT_FLAG_CENTER): the query's first row comes
    // off every row before anything is multiplied; distances and the bounding box's extent do not move, the expansion stops
    // cancelling.  A compile-time form: four more live registers push the plain kernels over their three-per-CU budget.
    const float4 mu = CENTER ? ld4(qdoc + dofs) : make_float4(0.f, 0.f, 0.f, 0.f);
    float* red = lds + wave * (T * T * 128);
    float* rednorm = lds + Lds<T>::kRed + wave * (T * 16);
    float* xp = lds + Lds<T>::kXp + wave * kXpWave;
    float4 mn = make_float4(INFINITY, INFINITY, INFINITY, INFINITY);
    float4 mx = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
    if constexpr (T == 1) {
        // One tile: issue every load up front -- the query rows first (L2-resident, they land early), then the
        // candidate rows from HBM -- and let the accumulation start on y[0] while y[1..7] are still in flight
        // (the j-outer loops below wait per row with counted vmcnt).  Both query halves are resident, so the
        // second half starts without another exposed load latency.
        float4 x0[4], x1[4], y[8];
        load_rows<4, BBOX, CENTER>(x0, qdoc, 0, q_avail, dofs, q_box, mn, mx, mu);
        load_rows<4, BBOX, CENTER>(x1, qdoc, 4, q_avail, dofs, q_box, mn, mx, mu);
        load_rows<8, BBOX, CENTER>(y, cdoc, 0, c_avail, dofs, c_box, mn, mx, mu);
        half_tile_partials<NEED_G, NEED_D2>(x0, y, red, xp, lane);
        half_tile_partials<NEED_G, NEED_D2>(x1, y, red + 32, xp, lane);
        if (NEED_G) {
            float nrm[16];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                nrm[i] = sq4(x0[i]);
                nrm[4 + i] = sq4(x1[i]);
                nrm[8 + i] = sq4(y[i]);
                nrm[12 + i] = sq4(y[4 + i]);
            }
            const float r = lds_wave_reduce<16>(nrm, xp, lane);
            if ((lane & 3) == 0) rednorm[lane >> 2] = r;
        }
    } else {
    // whole 8 x 8 tiles past a document's rows are skipped (CSR documents: `avail` = the document's own length; consumers
    // never read those tiles' sums -- finish_pair, l2max_kernel).  Row norms: the query tile's with the first candidate tile,
    // the candidate tile's with the first query tile.
    const int Tq = min(T, max(1, (q_avail + 7) >> 3)), Tc = min(T, max(1, (c_avail + 7) >> 3));
#pragma unroll 1
    for (int tj = 0; tj < Tc; ++tj) {
        float4 y[8];
        load_rows<8, BBOX, CENTER>(y, cdoc, tj * 8, c_avail, dofs, c_box, mn, mx, mu);
#pragma unroll 1
        for (int ti = 0; ti < Tq; ++ti) {
            float nrm[16];  // |x_i|^2 of the 8 query rows, |y_j|^2 of the 8 candidate rows (first row / column of tiles only)
            const bool want_norms = NEED_G && (ti == 0 || tj == 0);
#pragma unroll 1
            for (int half = 0; half < 2; ++half) {
                float4 x[4];
                load_rows<4, BBOX, CENTER>(x, qdoc, ti * 8 + half * 4, q_avail, dofs, q_box, mn, mx, mu);  // min/max idempotent
                half_tile_partials<NEED_G, NEED_D2>(x, y, red + (ti * T + tj) * 128 + half * 32, xp, lane);
                if (want_norms) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        if (half == 0) {
                            nrm[i] = sq4(x[i]);
                            nrm[8 + i] = sq4(y[i]);
                            nrm[12 + i] = sq4(y[4 + i]);
                        } else {
                            nrm[4 + i] = sq4(x[i]);
                        }
                    }
                }
            }
            if (want_norms) {
                const float r = lds_wave_reduce<16>(nrm, xp, lane);
                const int e = lane >> 2;                  // 0 .. 7: query rows of tile ti, 8 .. 15: candidate rows of tile tj
                if ((lane & 3) == 0 && (e < 8 ? tj == 0 : ti == 0)) rednorm[(e < 8 ? ti : tj) * 16 + e] = r;
            }
        }
    }
    }
    if (BBOX) {
        const float dx = mx.x - mn.x, dy = mx.y - mn.y, dz = mx.z - mn.z, dw = mx.w - mn.w;
        const float s = wave_sum(fmaf(dw, dw, fmaf(dz, dz, fmaf(dy, dy, dx * dx))));
        if (lane == 0) lds[Lds<T>::kRed + Lds<T>::kNorm + wave] = s;
    }
}

// ---------------------------------------------------------------------------------------------
// max-sim kernel (A9)
// ---------------------------------------------------------------------------------------------
template <int T>
__global__ void __launch_bounds__(kBlock, 3) l2max_kernel(ScoreArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t c_idx = blockIdx.x;
    const int c_len = a.c.len[c_idx];
    const int c_avail = a.c.ext > 0 ? a.c.ext : c_len;
    const float* cdoc = a.c.rows + (size_t)a.c.start[c_idx] * kD;
    // one query per candidate (PAIRED: the candidate's own index; MAPPED: its job's) or a block of queries (CROSS)
    const bool one_q = a.pairing != ASPIRE_PAIR_CROSS;
    const int64_t q_begin = a.pairing == ASPIRE_PAIR_PAIRED ? c_idx : a.pairing == kPairMapped ? (int64_t)a.qmap[c_idx]
                                                                                                : (int64_t)blockIdx.y * a.q_per_block;
    const int64_t q_end = one_q ? q_begin + 1 : min(a.q.n, q_begin + a.q_per_block);
    const int li = lane >> 3, lj = lane & 7;
    for (int64_t q_idx = q_begin; q_idx < q_end; ++q_idx) {
        const int q_len = a.q.len[q_idx];
        const int q_avail = a.q.ext > 0 ? a.q.ext : q_len;
        const float* qdoc = a.q.rows + (size_t)a.q.start[q_idx] * kD;
        const bool mm = use_mm_formula(a.cdist_mode, q_avail, c_avail);
        if (mm) {
            pair_partials<T, true, false, false>(qdoc, q_avail, 0, cdoc, c_avail, 0, lds, wave, lane);
        } else {
            pair_partials<T, false, true, false>(qdoc, q_avail, 0, cdoc, c_avail, 0, lds, wave, lane);
        }
        __syncthreads();
        if (wave == 0) {
            const int64_t p = one_q ? c_idx : q_idx * a.c.n + c_idx;
            float negv[T][T];
            bool val[T][T];
#pragma unroll
            for (int ta = 0; ta < T; ++ta)
#pragma unroll
                for (int tb = 0; tb < T; ++tb) {
                    const int i = ta * 8 + li, j = tb * 8 + lj;
                    const float* r = lds + (ta * T + tb) * 128;
                    float d2;
                    if (T > 1 && (ta * 8 >= q_avail || tb * 8 >= c_avail)) {
                        d2 = 0.f;                       // a tile pair_partials skipped: no sums in LDS, no valid entry
                    } else if (mm) {
                        float g = 0.f, xx = 0.f, yy = 0.f;
#pragma unroll
                        for (int w = 0; w < kWaves; ++w) {
                            g += r[w * T * T * 128 + lane];
                            xx += lds[Lds<T>::kRed + w * T * 16 + ta * 16 + li];
                            yy += lds[Lds<T>::kRed + w * T * 16 + tb * 16 + 8 + lj];
                        }
                        const float sqv = fmaf(-2.f, g, xx) + yy, ns = xx + yy;
                        d2 = fmaxf(sqv, 0.f);
                        // (under this formula too -- the rule: exact_d2.h.  Rare: the lane walks the two rows itself, form C)
                        if (i < q_len && j < c_len && expansion_cancels(sqv, ns)) {
                            const float* xr = qdoc + (size_t)i * kD;
                            const float* yr = cdoc + (size_t)j * kD;
                            d2 = lane_d2([=](int d) { return ld4(xr + d); }, [=](int d) { return ld4(yr + d); });
                        }
                    } else {
                        d2 = 0.f;
#pragma unroll
                        for (int w = 0; w < kWaves; ++w) d2 += r[w * T * T * 128 + 64 + lane];
                    }
                    negv[ta][tb] = -sqrtf(d2);
                    val[ta][tb] = i < q_len && j < c_len;
                    if (a.out_pairsims && i < a.q.ext && j < a.c.ext)
                        a.out_pairsims[(p * a.q.ext + i) * a.c.ext + j] =
                            negv[ta][tb] + ((val[ta][tb] || a.agg == ASPIRE_AGG_ATTENTION) ? 0.f : -10e8f);
                }
            float score;
            if (a.agg == ASPIRE_AGG_MAX) {
                float best = -INFINITY;
#pragma unroll
                for (int ta = 0; ta < T; ++ta)
#pragma unroll
                    for (int tb = 0; tb < T; ++tb)
                        if (val[ta][tb]) best = fmaxf(best, negv[ta][tb]);
                score = wave_max(best);
            } else if (a.agg == ASPIRE_AGG_TOP2) {
                // torch.topk(k=2) over the padded block: masked entries take part with -cdist - 10e8
                float m1 = -INFINITY, m2 = -INFINITY;
                auto push = [&](float v) {
                    m2 = fmaxf(m2, fminf(m1, v));
                    m1 = fmaxf(m1, v);
                };
#pragma unroll
                for (int ta = 0; ta < T; ++ta)
#pragma unroll
                    for (int tb = 0; tb < T; ++tb) {
                        const int i = ta * 8 + li, j = tb * 8 + lj;
                        if (val[ta][tb]) push(negv[ta][tb]);
                        else if (i < a.q.ext && j < a.c.ext) push(negv[ta][tb] + -10e8f);
                    }
#pragma unroll
                for (int m = 1; m < 64; m <<= 1) {
                    const float o1 = __shfl_xor(m1, m), o2 = __shfl_xor(m2, m);
                    m2 = fmaxf(fminf(m1, o1), fmaxf(m2, o2));
                    m1 = fmaxf(m1, o1);
                }
                if (m2 == -INFINITY) m2 = -10e8f;   // no padded extent and a 1 x 1 pair
                score = m1 + m2;
            } else {
                // masked 2-D soft-max of -d / temp over the valid block, then sum p * (-d)
                const float temp = (float)a.temp;
                float mx = -INFINITY;
#pragma unroll
                for (int ta = 0; ta < T; ++ta)
#pragma unroll
                    for (int tb = 0; tb < T; ++tb)
                        if (val[ta][tb]) mx = fmaxf(mx, negv[ta][tb] / temp);
                mx = wave_max(mx);
                float e[T][T], se = 0.f, sn = 0.f;
#pragma unroll
                for (int ta = 0; ta < T; ++ta)
#pragma unroll
                    for (int tb = 0; tb < T; ++tb) {
                        e[ta][tb] = val[ta][tb] ? expf(negv[ta][tb] / temp - mx) : 0.f;
                        se += e[ta][tb];
                        sn = fmaf(e[ta][tb], negv[ta][tb], sn);
                    }
                se = wave_sum(se);
                sn = wave_sum(sn);
                score = sn / se;
                if (a.out_plan) {
#pragma unroll
                    for (int ta = 0; ta < T; ++ta)
#pragma unroll
                        for (int tb = 0; tb < T; ++tb) {
                            const int i = ta * 8 + li, j = tb * 8 + lj;
                            if (i < a.q.ext && j < a.c.ext) a.out_plan[(p * a.q.ext + i) * a.c.ext + j] = e[ta][tb] / se;
                        }
                }
            }
            if (lane == 0) a.scores[p] = score;
        }
        __syncthreads();
    }
}

// After the three waves' partial sums of one pair met in LDS: all 192 threads finish the entries
// (sum of partials, both L2 formulas) and store them to the pair's workspace slot.
template <int T, bool DIRECT = true>
__device__ __forceinline__ void finish_pair(const float* lds, bool mm, bool want_diam, const PairWs<T>& ws, int64_t slot,
                                            const float* qdoc = nullptr, const float* cdoc = nullptr, int q_len = 0, int c_len = 0,
                                            int q_avail = 8 * T, int c_avail = 8 * T) {
    for (int e = threadIdx.x; e < 64 * T * T; e += kBlock) {
        const int tile = e >> 6, l = e & 63, ta = tile / T, tb = tile % T, li = l >> 3, lj = l & 7;
        const float* r = lds + tile * 128;
        if (T > 1 && (ta * 8 >= q_avail || tb * 8 >= c_avail)) {
            // pair_partials skipped this tile (no row of one side reaches it); the solvers mask it
            const int64_t o = slot * (64 * T * T) + (ta * 8 + li) * (8 * T) + tb * 8 + lj;
            ws.cost[o] = 1.f;
            ws.neg[o] = -1.f;
            continue;
        }
        float g = 0.f, d2 = 0.f, xx = 0.f, yy = 0.f;
#pragma unroll
        for (int w = 0; w < kWaves; ++w) {
            g += r[w * T * T * 128 + l];
            if (DIRECT) d2 += r[w * T * T * 128 + 64 + l];
            xx += lds[Lds<T>::kRed + w * T * 16 + ta * 16 + li];
            yy += lds[Lds<T>::kRed + w * T * 16 + tb * 16 + 8 + lj];
        }
        const float sq = fmaf(-2.f, g, xx) + yy;
        const int64_t o = slot * (64 * T * T) + (ta * 8 + li) * (8 * T) + tb * 8 + lj;
        // geomloss's cost: its expansion -- except where that cancels (the test the streaming kernels use), where the exact sum
        // stands in: what the reference's own formula gives in float64 (in fp32 it returns the square root of rounding noise there)
        float costv = cost_of_d2(sq);
        if constexpr (DIRECT) {
            const float ns = xx + yy;
            const bool cancels = expansion_cancels(sq, ns);
            if (cancels) costv = cost_of_d2(d2);
            ws.cost[o] = costv;
            ws.neg[o] = (mm && !cancels) ? neg_of_expansion(sq) : -sqrtf(d2);      // (a cancelling entry from the exact sum under either formula: exact_d2.h)
        } else {
            // only x.y was accumulated (see pair_cost1_kernel): -cdist from the expansion, except where it cancels
            const int i = ta * 8 + li, j = tb * 8 + lj;
            const float ns = xx + yy;
            float negv = neg_of_expansion(sq);
            if (i < q_len && j < c_len && expansion_cancels(sq, ns)) {   // rare: this thread walks the two rows itself (exact_d2.h, form C)
                const float* xr = qdoc + (size_t)i * kD;
                const float* yr = cdoc + (size_t)j * kD;
                const float d2x = lane_d2([=](int d) { return ld4(xr + d); }, [=](int d) { return ld4(yr + d); });
                negv = -sqrtf(d2x);
                costv = cost_of_d2(d2x);
            }
            ws.cost[o] = costv;
            ws.neg[o] = negv;
        }
    }
    if (want_diam && threadIdx.x == 0) {
        const float* dd = lds + Lds<T>::kRed + Lds<T>::kNorm;
        ws.diam2[slot] = dd[0] + dd[1] + dd[2];
    }
}

// Kernel 1 of the otAspire path: pairwise sentence costs of the pairs of one chunk of candidates
// [a.cand0, a.cand1) -> workspace.  Streams every candidate row once; HBM bound for few queries.
// DIRECT: both L2 formulas accumulated (padded reference tensors: their pair matrices are compared at 1e-5).  !DIRECT
// (CSR inputs): x.y only, -cdist from the expansion with the cancelled entries redone -- half the arithmetic and
// half the cross-lane reductions of the T x T tile loop.
template <int T, bool DIRECT, bool CENTER = false>
__global__ void __launch_bounds__(kBlock, 3) pair_cost_kernel(ScoreArgs a, PairWs<T> ws) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const bool paired = a.pairing != ASPIRE_PAIR_CROSS;          // one query per candidate (PAIRED, MAPPED)
    const int64_t c_idx = a.cand0 + blockIdx.x;
    const int64_t ncand = a.cand1 - a.cand0;
    const int64_t q_own = a.pairing == kPairMapped ? (int64_t)a.qmap[c_idx] : c_idx;
    const int64_t q_begin = paired ? q_own : (int64_t)blockIdx.y * a.q_per_block;
    const int64_t q_end = paired ? q_own + 1 : min(a.q.n, q_begin + a.q_per_block);
    const bool own_diam = a.diameter == nullptr;
    const int c_len = a.c.len[c_idx];
    const int c_avail = a.c.ext > 0 ? a.c.ext : c_len;
    const float* cdoc = a.c.rows + (size_t)a.c.start[c_idx] * kD;
    for (int64_t q_idx = q_begin; q_idx < q_end; ++q_idx) {
        const int q_len = a.q.len[q_idx];
        const int q_avail = a.q.ext > 0 ? a.q.ext : q_len;
        const float* qdoc = a.q.rows + (size_t)a.q.start[q_idx] * kD;
        if (own_diam) {
            pair_partials<T, true, DIRECT, true, CENTER>(qdoc, q_avail, q_len, cdoc, c_avail, c_len, lds, wave, lane);
        } else {
            pair_partials<T, true, DIRECT, false, CENTER>(qdoc, q_avail, 0, cdoc, c_avail, 0, lds, wave, lane);
        }
        __syncthreads();
        const int64_t slot = paired ? (c_idx - a.cand0) : q_idx * ncand + (c_idx - a.cand0);
        finish_pair<T, DIRECT>(lds, use_mm_formula(a.cdist_mode, q_avail, c_avail), own_diam, ws, slot, qdoc, cdoc, q_len, c_len, q_avail,
                               c_avail);
        __syncthreads();
    }
}

// Kernel 1, single-tile (<= 8 sentence rows on both sides) persistent form: a fixed grid of workgroups walks the
// items (candidate-major pairs) with a stride of gridDim.x, and the NEXT item's 16 rows are already in flight
// (64 more VGPRs per lane) while the current item is accumulated, reduced and written -- the HBM latency that
// the one-item-per-workgroup form exposes at the head of every workgroup is paid once per workgroup instead.
struct RowSet {
    float4 x0[4], x1[4], y[8];
};

// Rows beyond a document's length are loaded as COPIES OF ITS LAST ROW (row index clamped): entries that involve
// them are masked downstream, and duplicates leave the bounding box unchanged, so the box needs no per-row
// predicate.  (Only used when ext == 0; padded tensors take the general kernel, which reads the real pad rows.)
// `item` = (sub-tile, pair): T * T sub-tiles of 8 x 8 entries per pair (1 for documents of <= 8 rows), the pair index
// fastest.  Sub-tile (ta, tb) takes query rows 8 ta .. and candidate rows 8 tb ...
// Plain global loads with per-row vector addresses (a buffer-descriptor form was measured: the scheduler spreads it
// over all 256 registers of its budget -- 197 here -- and a 256-register kernel shares a SIMD with nothing).
__device__ __forceinline__ void load_item(RowSet& r, const ScoreArgs& a, uint32_t item, uint32_t nq, int dofs,
                                          int& q_len, int& c_len, uint32_t T) {
    const uint32_t npairs = (uint32_t)(a.cand1 - a.cand0) * nq;
    const uint32_t tile = T == 1 ? 0 : item / npairs;        // pair index fastest: a pair's sub-tiles go to different workgroups
    const uint32_t pair = item - tile * npairs, ta = tile / T, tb = tile - ta * T;
    const uint32_t c_loc = nq == 1 ? pair : pair / nq;
    const int64_t c_idx = a.cand0 + c_loc;
    const int64_t q_idx = a.pairing == ASPIRE_PAIR_PAIRED ? c_idx
                          : a.pairing == kPairMapped      ? (int64_t)a.qmap[c_idx]
                                                          : (nq == 1 ? 0 : pair - c_loc * nq);
    const int i0 = 8 * ta, j0 = 8 * tb;
    // `item` is workgroup-uniform: the lengths go to scalar registers (as vector loads they held four VGPRs across the
    // item loop and took pair_cost1_kernel to 201 registers, over the co-residency budget above)
    c_len = __builtin_amdgcn_readfirstlane(a.c.len[c_idx]);
    q_len = __builtin_amdgcn_readfirstlane(a.q.len[q_idx]);
    const float* cdoc = a.c.rows + (size_t)a.c.start[c_idx] * kD + dofs;
    const float* qdoc = a.q.rows + (size_t)a.q.start[q_idx] * kD + dofs;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        r.x0[i] = ld4(qdoc + (size_t)min(i0 + i, q_len - 1) * kD);
        r.x1[i] = ld4(qdoc + (size_t)min(i0 + 4 + i, q_len - 1) * kD);
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) r.y[j] = ld4_stream(cdoc + (size_t)min(j0 + j, c_len - 1) * kD);
}

__device__ __forceinline__ float box_partial(const RowSet& r) {
    float4 mn = r.y[0], mx = r.y[0];
    auto upd = [&](const float4& v) {
        mn.x = fminf(mn.x, v.x); mn.y = fminf(mn.y, v.y); mn.z = fminf(mn.z, v.z); mn.w = fminf(mn.w, v.w);
        mx.x = fmaxf(mx.x, v.x); mx.y = fmaxf(mx.y, v.y); mx.z = fmaxf(mx.z, v.z); mx.w = fmaxf(mx.w, v.w);
    };
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        upd(r.x0[i]);
        upd(r.x1[i]);
    }
#pragma unroll
    for (int j = 1; j < 8; ++j) upd(r.y[j]);
    const float dx = mx.x - mn.x, dy = mx.y - mn.y, dz = mx.z - mn.z, dw = mx.w - mn.w;
    return fmaf(dw, dw, fmaf(dz, dz, fmaf(dy, dy, dx * dx)));
}

// The persistent, software-pipelined form: the next item's rows are in flight in a second register set while the
// current item is accumulated, reduced and written.
// SUB: documents of more than 8 rows, (sub-tile, pair) items; !SUB keeps the one-tile case free of the sub-tile
// arithmetic.  Register budgets decide how these kernels share a SIMD with OTHER launches (independent calls on other
// streams): at 197 registers two of these waves leave room for two 52-register Sinkhorn waves; at 256 nothing fits beside
// them and overlapped throughput fell from ~110 to ~70 M alignments/s with every kernel's own time unchanged.
// tests/test_abi_cpu.py pins the budgets.  (Superseded forms -- one register set with buffer loads, a matrix-core
// form, cost + solve fused per workgroup -- are described in NOTES.md "Tried and dropped".)
template <bool SUB>
__device__ __forceinline__ void pair_cost1_body(const ScoreArgs& a, const PairWs<1>& ws, uint32_t T_rt, float* lds) {
    const uint32_t T = SUB ? T_rt : 1u;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int dofs = wave * 256 + lane * 4;
    const bool paired = a.pairing != ASPIRE_PAIR_CROSS;          // one query per candidate (PAIRED, MAPPED)
    // 32-bit item arithmetic: a chunk holds at most workspace / 516 B < 2^31 pairs, and 64-bit division costs
    // hundreds of cycles per item on this hardware.
    const uint32_t nq = paired ? 1u : (uint32_t)a.q.n;
    auto query_of = [&](int64_t c_idx, uint32_t q_loc) -> int64_t {
        return a.pairing == ASPIRE_PAIR_PAIRED ? c_idx : a.pairing == kPairMapped ? (int64_t)a.qmap[c_idx] : (int64_t)q_loc;
    };
    const uint32_t ncand = (uint32_t)(a.cand1 - a.cand0);
    const uint32_t tt = T * T, ld_e = 8 * T, n_ent = 64 * tt;      // sub-tiles per pair, row stride and entries of a pair's slot
    const uint32_t n_items = ncand * nq * tt;
    const bool own_diam = a.diameter == nullptr;
    float* red = lds + wave * 128;
    float* rednorm = lds + Lds<1>::kRed + wave * 16;
    float* xp = lds + Lds<1>::kXp + wave * kXpWave;

    // One item: accumulate, reduce, finish, hand over.  `r` is one of two register sets that take turns (the loop
    // below is unrolled by two so that the set being prefetched into is never copied).
    auto process = [&](RowSet& rs, int q_len, int c_len, uint32_t item) {
        if (a.center) {          // ASPIRE_OT_FLAG_CENTER: the tile's first query row comes off every row (see pair_partials)
            const float4 mu = rs.x0[0];
            auto sub = [&](float4& v) { v.x -= mu.x; v.y -= mu.y; v.z -= mu.z; v.w -= mu.w; };
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                sub(rs.x0[i]);
                sub(rs.x1[i]);
            }
#pragma unroll
            for (int j = 0; j < 8; ++j) sub(rs.y[j]);
        }
        // ---- accumulate + reduce the current item (register operands only).  Only the x.y sums are accumulated:
        // geomloss's cost is the expansion anyway, and torch.cdist's direct (x - y)^2 form (the marginals' -cdist)
        // is met by the same expansion to a few 1e-5 except where it cancels -- those entries (d^2 below 1e-4 of the
        // squared norm sum; none on unrelated vectors) are redone coordinate by coordinate below.  Dropping the
        // second set of 32 accumulators and its cross-lane reduction is 2/3 of this kernel's VALU work, which at
        // ~1000 pairs is what the kernel's time is made of.
        half_tile_partials<true, false>(rs.x0, rs.y, red, xp, lane);
        half_tile_partials<true, false>(rs.x1, rs.y, red + 32, xp, lane);
        {
            float nrm[16];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                nrm[i] = sq4(rs.x0[i]);
                nrm[4 + i] = sq4(rs.x1[i]);
                nrm[8 + i] = sq4(rs.y[i]);
                nrm[12 + i] = sq4(rs.y[4 + i]);
            }
            const float r = lds_wave_reduce<16>(nrm, xp, lane);
            if ((lane & 3) == 0) rednorm[lane >> 2] = r;
        }
        const uint32_t npairs = ncand * nq;
        const uint32_t tile = tt == 1 ? 0 : item / npairs;
        const uint32_t pair = item - tile * npairs, ta = tile / T, tb = tile - ta * T;
        const uint32_t c_loc = nq == 1 ? pair : pair / nq;
        const uint32_t q_loc = nq == 1 ? 0 : pair - c_loc * nq;
        if (own_diam && tile == 0) {
            float sbox;
            if (tt == 1) {
                sbox = wave_sum(box_partial(rs));
            } else {
                // long documents: the bounding box spans ALL rows of both documents; the pair's first sub-tile walks them
                const int64_t c_idx = a.cand0 + c_loc;
                const int64_t q_idx = query_of(c_idx, q_loc);
                const float* qd = a.q.rows + (size_t)a.q.start[q_idx] * kD + dofs;
                const float* cd = a.c.rows + (size_t)a.c.start[c_idx] * kD + dofs;
                float4 mn = ld4(qd), mx = mn;
                auto upd = [&](const float4& v) {
                    mn.x = fminf(mn.x, v.x); mn.y = fminf(mn.y, v.y); mn.z = fminf(mn.z, v.z); mn.w = fminf(mn.w, v.w);
                    mx.x = fmaxf(mx.x, v.x); mx.y = fmaxf(mx.y, v.y); mx.z = fmaxf(mx.z, v.z); mx.w = fmaxf(mx.w, v.w);
                };
                auto walk = [&](const float* doc, int n) {     // eight independent loads in flight (rows clamp: idempotent)
                    for (int r0 = 0; r0 < n; r0 += 8) {
                        float4 v[8];
#pragma unroll
                        for (int k = 0; k < 8; ++k) v[k] = ld4(doc + (size_t)min(r0 + k, n - 1) * kD);
#pragma unroll
                        for (int k = 0; k < 8; ++k) upd(v[k]);
                    }
                };
                walk(qd, q_len);
                walk(cd, c_len);
                const float dx = mx.x - mn.x, dy = mx.y - mn.y, dz = mx.z - mn.z, dw = mx.w - mn.w;
                sbox = wave_sum(fmaf(dw, dw, fmaf(dz, dz, fmaf(dy, dy, dx * dx))));
            }
            if (lane == 0) lds[Lds<1>::kRed + Lds<1>::kNorm + wave] = sbox;
        }
        __syncthreads();
        const int64_t slot = paired ? (int64_t)c_loc : (int64_t)q_loc * ncand + c_loc;
        // A dedicated word: wave 0 rewrites it only after the NEXT item's first barrier, which every wave reaches only
        // after it has read this item's mask (it used to live in wave 0's reduction scratch, which wave 0 rewrites
        // at once when a workgroup walks several items).
        unsigned long long* redo_mask = reinterpret_cast<unsigned long long*>(lds + Lds<1>::kRedo);
        if (wave == 0) {
            const int li = lane >> 3, lj = lane & 7;
            float gsum = 0.f, xx = 0.f, yy = 0.f;
#pragma unroll
            for (int w = 0; w < kWaves; ++w) {
                gsum += lds[w * 128 + lane];
                xx += lds[Lds<1>::kRed + w * 16 + li];
                yy += lds[Lds<1>::kRed + w * 16 + 8 + lj];
            }
            const float sq = fmaf(-2.f, gsum, xx) + yy;
            const float ns = xx + yy;
            const int gi = 8 * ta + li, gj = 8 * tb + lj;                  // entry of the pair's 8T x 8T slot
            const bool redo = gi < q_len && gj < c_len && expansion_cancels(sq, ns);       // (the rule and the exact sum: exact_d2.h)
            const int64_t o = slot * n_ent + gi * ld_e + gj;
            if (!redo) {
                ws.cost[o] = cost_of_d2(sq);
                ws.neg[o] = neg_of_expansion(sq);
            }
            const unsigned long long m = __ballot(redo);
            if (lane == 0) {
                *redo_mask = m;
                if (own_diam && tile == 0) {
                    const float* dd = lds + Lds<1>::kRed + Lds<1>::kNorm;
                    ws.diam2[slot] = dd[0] + dd[1] + dd[2];
                }
            }
        }
        __syncthreads();
        {
            const unsigned long long todo = *redo_mask;     // workgroup-uniform
            if (__builtin_expect(todo != 0, 0)) {
                // 16 lanes (one DPP row) per flagged entry, 48 coordinates per lane, twelve entries at a time over
                // the three waves, no barriers: with real sentence vectors a few entries per pair can be this close
                const int64_t c_idx = a.cand0 + c_loc;
                const int64_t q_idx = query_of(c_idx, q_loc);
                const float* qdoc = a.q.rows + (size_t)a.q.start[q_idx] * kD;
                const float* cdoc = a.c.rows + (size_t)a.c.start[c_idx] * kD;
                const int n_flag = __builtin_popcountll(todo), l16 = lane & 15;
                for (int base = wave * 4; base < n_flag; base += 4 * kWaves) {
                    const int my = base + (lane >> 4);
                    const bool live = my < n_flag;
                    unsigned long long m = todo;
                    for (int t = 0; t < (live ? my : 0); ++t) m &= m - 1;      // drop the first `my` set bits
                    const int e = __builtin_ctzll(m);
                    const int gi = 8 * ta + (e >> 3), gj = 8 * tb + (e & 7);
                    const float* xr = qdoc + (size_t)gi * kD + 4 * l16;
                    const float* yr = cdoc + (size_t)gj * kD + 4 * l16;
                    const float part = row16_d2([=](int d) { return ld4(xr + d); }, [=](int d) { return ld4(yr + d); });
                    if (live && l16 == 0) {       // geomloss's cost from the same exact sum
                        ws.neg[slot * n_ent + gi * ld_e + gj] = -sqrtf(part);
                        ws.cost[slot * n_ent + gi * ld_e + gj] = cost_of_d2(part);
                    }
                }
            }
        }
    };
    RowSet ra, rb;
    int qa = 0, ca = 0, qb = 0, cb = 0;
    const uint32_t stride = gridDim.x;
    uint32_t item = blockIdx.x;
    if (item < n_items) load_item(ra, a, item, nq, dofs, qa, ca, T);
    while (item < n_items) {
        const uint32_t n1 = item + stride;
        if (n1 < n_items) load_item(rb, a, n1, nq, dofs, qb, cb, T);     // in flight under this item's arithmetic
        process(ra, qa, ca, item);
        if (n1 >= n_items) break;
        const uint32_t n2 = n1 + stride;
        if (n2 < n_items) load_item(ra, a, n2, nq, dofs, qa, ca, T);
        process(rb, qb, cb, n1);
        item = n2;
    }
}
__global__ void __launch_bounds__(kBlock, 2) pair_cost1_kernel(ScoreArgs a, PairWs<1> ws, uint32_t T_rt) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    pair_cost1_body<false>(a, ws, T_rt, lds);
}
// The sub-tile form, capped at 216 registers (amdgpu_num_vgpr counts HALF registers on gfx950: 108 -> 216; uncapped it
// takes 256 and no other launch's waves share a SIMD with it).
#ifndef SUB_CAP
#define SUB_CAP 108
#endif
__global__ void __launch_bounds__(kBlock, 2) __attribute__((amdgpu_num_vgpr(SUB_CAP)))
pair_cost1_sub_kernel(ScoreArgs a, PairWs<1> ws, uint32_t T_rt) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    pair_cost1_body<true>(a, ws, T_rt, lds);
}

// ---------------------------------------------------------------------------------------------
// Kernel 1, tiled form for documents of <= 8 sentence rows (T == 1, CSR inputs).
//
// The accumulate-then-reduce kernels above give every lane a slice of the 768 coordinates and all 64 (i,j)
// pairs, so each pair costs a 64-lane reduction of 128 accumulators -- on gfx950 that reduction (LDS transpose or
// permlane butterfly) costs several times the multiply-adds it serves.  Here the roles are swapped, GEMM style:
// a lane OWNS R x R entries (i,j) of a pair and walks all 768 coordinates itself, so its accumulators are finished
// sums and nothing is reduced across lanes.  The sentence rows are staged through LDS 16-byte chunk by chunk
// (coalesced global_load_dwordx4 -> ds_write_b128; row stride padded so the operand reads are conflict free) and
// re-read as ds_read_b128 broadcasts.  One wave handles NC = R*R = 4 candidates against one query, 16 lanes each: a
// lane owns the 2x2 block (2li+a, 2lj+b); stages of 64 coordinates (the 16 lanes of candidate p stage its 8 rows and
// query rows 2p, 2p+1).  Every wave of the 4-wave workgroup takes its own items.
// While staging, the lane that holds all 8 rows of a candidate for one chunk also forms that chunk's bounding-box
// term (geomloss diameter) and the row norms, so those cost no extra pass either.
// ---------------------------------------------------------------------------------------------
struct TileCfg {
    static constexpr int kR = 2;                   // a lane's block of entries is kR x kR
    static constexpr int kNC = kR * kR;            // candidates per wave
    static constexpr int kLanesPerCand = 64 / kNC;
    static constexpr int kGroups = 4;              // staging lane groups
    static constexpr int kCh = 64 / kGroups;       // 16-byte chunks per row per stage
    static constexpr int kStages = 192 / kCh;
    static constexpr int kRowStride = 4 * kCh + 4; // floats; (kRowStride / 4) is odd -> rows land on distinct bank slots
    static constexpr int kRows = 8 + 8 * kNC;      // staged rows: 8 query + 8 per candidate
    static constexpr int kNormLd = 68;
    static constexpr int kLdsFloats = kRows * kRowStride + 16 * kNormLd;   // + norm / box scratch
    static constexpr int kXRows = 2;               // query rows staged by one lane
};

// per-coordinate bounding box of each query's valid rows: qbox[q][0][768] = min, qbox[q][1][768] = max
__global__ void __launch_bounds__(192) doc_box_kernel(RepSet d, float* __restrict__ box) {
    const int64_t k = blockIdx.x;
    const int n = d.len[k];
    const float* doc = d.rows + (size_t)d.start[k] * kD + threadIdx.x * 4;
    float4 mn, mx;
    doc_box_chunk(doc, n, mn, mx);
    *reinterpret_cast<float4*>(box + k * 2 * kD + threadIdx.x * 4) = mn;
    *reinterpret_cast<float4*>(box + k * 2 * kD + kD + threadIdx.x * 4) = mx;
}

// gate[0] += pairs of this launch that hold a document of more than 8 rows (MAPPED: candidate p against query qmap[p]; CROSS:
// one query).  The counter is zeroed on the stream in front of it.
__global__ void __launch_bounds__(256) long_pair_census_kernel(ScoreArgs a, int32_t* gate) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    int is_long = 0;
    if (p < a.c.n) {
        const int64_t q_idx = a.pairing == kPairMapped ? (int64_t)a.qmap[p] : 0;
        is_long = a.c.len[p] > 8 || a.q.len[q_idx] > 8;
    }
    const int n = __popcll(__ballot(is_long));
    if ((threadIdx.x & 63) == 0 && n) atomicAdd(gate, n);
}

__global__ void __launch_bounds__(256) pair_tile_kernel(ScoreArgs a, PairWs<1> ws, const float* __restrict__ qbox) {
    using C = TileCfg;
    constexpr int R = C::kR;
    extern __shared__ __attribute__((aligned(16))) float lds_all[];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    float* lds = lds_all + wave * C::kLdsFloats;
    float* nscr = lds + C::kRows * C::kRowStride;       // [16][kNormLd]: norm partials
    const bool paired = a.pairing == ASPIRE_PAIR_PAIRED;
    const bool mapped = a.pairing == kPairMapped;                // batched jobs: items are the groups of four of jobs [job0, job1)
    const bool own_diam = a.diameter == nullptr;
    const uint32_t nq = (paired || mapped) ? 1u : (uint32_t)a.q.n;
    const uint32_t ncand = (uint32_t)(a.cand1 - a.cand0);
    const uint32_t ngroups = (ncand + C::kNC - 1) / C::kNC;
    const uint32_t item_lo = mapped ? (uint32_t)a.grp_off[a.job0] : 0u;
    const uint32_t n_items = mapped ? (uint32_t)a.grp_off[a.job1] : ngroups * nq;   // item = (candidate group, query), group-major
    const uint32_t first = item_lo + blockIdx.x * 4 + wave;
    const uint32_t stride = gridDim.x * 4;

    // lane roles ------------------------------------------------------------------------------------------
    const int p = lane / C::kLanesPerCand;                       // candidate of this lane (compute AND staging)
    const int lp = lane % C::kLanesPerCand;
    const int li = lp / (8 / R), lj = lp % (8 / R);
    const int sg = lane / C::kCh, sc = lane % C::kCh;            // staging group, staging chunk: group g stages the 8 rows of candidate g and query rows 2g, 2g+1

    for (uint32_t item = first; item < n_items; item += stride) {
        const uint32_t cg = nq == 1 ? item : item / nq;
        uint32_t q_loc = nq == 1 ? 0 : item - cg * nq;
        uint32_t c_loc0 = cg * C::kNC;                                         // first candidate of the group
        uint32_t c_end = ncand;                                                // candidates of the group stop here
        if (mapped) {
            q_loc = (uint32_t)a.grp_job[item];
            c_loc0 = (uint32_t)a.job_off[q_loc] + (item - (uint32_t)a.grp_off[q_loc]) * C::kNC;
            c_end = (uint32_t)a.job_off[q_loc + 1];
        }
        const uint32_t my_c_loc = min(c_loc0 + (uint32_t)p, c_end - 1);   // tail groups: clamp (duplicate work, not stored)
        const bool my_c_real = c_loc0 + (uint32_t)p < c_end;
        const int64_t c_idx = a.cand0 + my_c_loc;
        const int64_t q_idx = paired ? c_idx : (int64_t)q_loc;
        const int c_len = a.c.len[c_idx], q_len = a.q.len[q_idx];
        const float* qdoc = a.q.rows + (size_t)a.q.start[q_idx] * kD;
        // staging source of this lane (pad rows clamp to the last valid row: masked downstream, box-neutral)
        const int64_t sy_idx = a.cand0 + min(c_loc0 + (uint32_t)sg, c_end - 1);
        const int sy_len = a.c.len[sy_idx];
        const float* sy_doc = a.c.rows + (size_t)a.c.start[sy_idx] * kD;

        float accg[R][R];
#pragma unroll
        for (int x = 0; x < R; ++x)
#pragma unroll
            for (int y = 0; y < R; ++y) accg[x][y] = 0.f;
        float ny[8], nx[C::kXRows], dsq = 0.f;
#pragma unroll
        for (int k = 0; k < 8; ++k) ny[k] = 0.f;
#pragma unroll
        for (int k = 0; k < C::kXRows; ++k) nx[k] = 0.f;

        float4 vy[8], vx[C::kXRows], qmn, qmx;
        const float* qb = own_diam ? qbox + (size_t)q_idx * 2 * kD : sy_doc;
        const int qb_hi = own_diam ? kD : 0;
        auto issue_loads = [&](int st) {
            const int dofs = (st * C::kCh + sc) * 4;
#pragma unroll
            for (int j = 0; j < 8; ++j) vy[j] = ld4_stream(sy_doc + (size_t)min(j, sy_len - 1) * kD + dofs);
            // UNCONDITIONAL (with caller-supplied diameters the candidate's first row stands in and the box term
            // is unused): a branch around these two loads made the compiler wait for the row loads just issued
            // at the join -- every stage's HBM latency in series with its arithmetic (see fused.hip)
            qmn = ld4(qb + dofs);
            qmx = ld4(qb + qb_hi + dofs);
#pragma unroll
            for (int k = 0; k < C::kXRows; ++k) vx[k] = ld4(qdoc + (size_t)min(2 * sg + k, q_len - 1) * kD + dofs);
        };
        issue_loads(0);
#pragma unroll 1
        for (int st = 0; st < C::kStages; ++st) {
            // ---- stage: registers -> LDS, with box / norm side products; then the NEXT stage's loads go out so
            // that they fly under this stage's arithmetic (no extra registers: the rows were just consumed) ----
            float4 mn = vy[0], mx = vy[0];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                ny[j] += sq4(vy[j]);
                if (j > 0) {
                    mn.x = fminf(mn.x, vy[j].x); mn.y = fminf(mn.y, vy[j].y); mn.z = fminf(mn.z, vy[j].z); mn.w = fminf(mn.w, vy[j].w);
                    mx.x = fmaxf(mx.x, vy[j].x); mx.y = fmaxf(mx.y, vy[j].y); mx.z = fmaxf(mx.z, vy[j].z); mx.w = fmaxf(mx.w, vy[j].w);
                }
                *reinterpret_cast<float4*>(lds + (8 + sg * 8 + j) * C::kRowStride + sc * 4) = vy[j];
            }
            if (own_diam) {
                const float dx = fmaxf(mx.x, qmx.x) - fminf(mn.x, qmn.x), dy = fmaxf(mx.y, qmx.y) - fminf(mn.y, qmn.y);
                const float dz = fmaxf(mx.z, qmx.z) - fminf(mn.z, qmn.z), dw = fmaxf(mx.w, qmx.w) - fminf(mn.w, qmn.w);
                dsq += fmaf(dw, dw, fmaf(dz, dz, fmaf(dy, dy, dx * dx)));
            }
#pragma unroll
            for (int k = 0; k < C::kXRows; ++k) {
                nx[k] += sq4(vx[k]);
                *reinterpret_cast<float4*>(lds + (2 * sg + k) * C::kRowStride + sc * 4) = vx[k];
            }
            if (st + 1 < C::kStages) issue_loads(st + 1);
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            // ---- accumulate: every lane walks the staged chunks for its own R x R entries ----------------------
            const float* xr = lds + (R * li) * C::kRowStride;
            const float* yr = lds + (8 + p * 8 + R * lj) * C::kRowStride;
#pragma unroll 1
            for (int c = 0; c < C::kCh; c += 2) {
              // two chunks per trip: the second chunk's LDS reads are in flight under the first chunk's arithmetic
#pragma unroll
              for (int cc = 0; cc < 2; ++cc) {
                float4 xv[R], yv[R];
#pragma unroll
                for (int x = 0; x < R; ++x) xv[x] = *reinterpret_cast<const float4*>(xr + x * C::kRowStride + (c + cc) * 4);
#pragma unroll
                for (int y = 0; y < R; ++y) yv[y] = *reinterpret_cast<const float4*>(yr + y * C::kRowStride + (c + cc) * 4);
#pragma unroll
                for (int x = 0; x < R; ++x)
#pragma unroll
                    for (int y = 0; y < R; ++y) {
                        accg[x][y] = fmaf(xv[x].w, yv[y].w, fmaf(xv[x].z, yv[y].z, fmaf(xv[x].y, yv[y].y, fmaf(xv[x].x, yv[y].x, accg[x][y]))));
                    }
              }
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");   // the stage buffer is rewritten next
            __builtin_amdgcn_wave_barrier();
        }

        // ---- norms and box: sum the staging lanes' partials through the scratch table nscr[value][lane] --------
        // value 0..7: |y_j|^2 partials of the lane's staged candidate; 8..8+kXRows-1: |x|^2 partials of its query rows
#pragma unroll
        for (int k = 0; k < 8; ++k) nscr[k * C::kNormLd + lane] = ny[k];
#pragma unroll
        for (int k = 0; k < C::kXRows; ++k) nscr[(8 + k) * C::kNormLd + lane] = nx[k];
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        auto table_sum = [&](int value, int lane0, int nlanes) {
            float t = 0.f;
            const float4* src = reinterpret_cast<const float4*>(lds_all + wave * C::kLdsFloats + C::kRows * C::kRowStride + value * C::kNormLd + lane0);
            for (int m = 0; m < nlanes / 4; ++m) {
                const float4 u = src[m];
                t += (u.x + u.y) + (u.z + u.w);
            }
            return t;
        };
        float xx[R], yy[R];
#pragma unroll
        for (int y = 0; y < R; ++y) yy[y] = table_sum(R * lj + y, p * 16, 16);
#pragma unroll
        for (int x = 0; x < R; ++x) xx[x] = table_sum(8 + ((R * li + x) & 1), ((R * li + x) >> 1) * 16, 16);
        float diam2 = 0.f;
        if (own_diam) {
            // box terms were formed by the lanes that staged candidate rows: sum them over that candidate's lanes
            float t = dsq;                       // 16 staging lanes of candidate sg == this lane's p (same grouping)
            t += lane_xor<1>(t); t += lane_xor<2>(t); t += lane_xor<4>(t); t += lane_xor<8>(t);
            diam2 = t;
        }

        // ---- finish the entries and hand them to the Sinkhorn kernel -----------------------------------------
        // Only x.y was accumulated: -cdist comes from the same expansion as the cost, and the entries where it cancels
        // (torch.cdist's direct formula differs there) are redone below.  See pair_cost1_kernel.
        // (the rule and the exact sum: exact_d2.h)
        const int64_t slot = (paired || mapped) ? (int64_t)my_c_loc : (int64_t)q_loc * ncand + my_c_loc;
        bool redo[R][R];
#pragma unroll
        for (int x = 0; x < R; ++x)
#pragma unroll
            for (int y = 0; y < R; ++y) {
                const int i = R * li + x, j = R * lj + y;
                const float sq = fmaf(-2.f, accg[x][y], xx[x]) + yy[y];
                const float ns = xx[x] + yy[y];
                redo[x][y] = my_c_real && i < q_len && j < c_len && expansion_cancels(sq, ns);
                if (my_c_real && !redo[x][y]) {
                    ws.cost[slot * 64 + i * 8 + j] = cost_of_d2(sq);
                    ws.neg[slot * 64 + i * 8 + j] = neg_of_expansion(sq);
                }
            }
        if (my_c_real && own_diam && lp == 0) ws.diam2[slot] = diam2;
        {
            // direct-formula redo, the whole wave on one entry, four entries per memory round trip: this kernel's own text of
            // exact_d2.h's redo_wave4 (through the helper it takes 212 registers instead of 210: NOTES.md)
            const int c_start_v = a.c.start[c_idx];
#pragma unroll
            for (int x = 0; x < R; ++x)
#pragma unroll
                for (int y = 0; y < R; ++y) {
                    unsigned long long wm = __ballot(redo[x][y]);
                    while (wm != 0) {
                        int owner[4];
                        float4 u[4][3], v[4][3];
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            owner[e] = wm != 0 ? (int)__builtin_ctzll(wm) : -1;
                            wm = wm != 0 ? wm & (wm - 1) : 0;
                        }
#pragma unroll
                        for (int e = 0; e < 4; ++e) {            // all 24 loads go out before the first is consumed
                            const int o = owner[e] >= 0 ? owner[e] : owner[0];
                            const int ol = o & 15, i = R * (ol >> 2) + x, j = R * (ol & 3) + y;
                            const int cs_e = __builtin_amdgcn_readlane(c_start_v, o);
                            const float* qrow = qdoc + (size_t)i * kD + 4 * lane;
                            const float* crow = a.c.rows + ((size_t)cs_e + j) * kD + 4 * lane;
#pragma unroll
                            for (int t = 0; t < 3; ++t) {
                                u[e][t] = ld4(qrow + 256 * t);
                                v[e][t] = ld4(crow + 256 * t);
                            }
                        }
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            const float part = wave_d2_part(u[e], v[e]);
                            if (owner[e] >= 0) {
                                const float tot = wave_sum(part);
                                const int ol = owner[e] & 15, i = R * (ol >> 2) + x, j = R * (ol & 3) + y;
                                if (lane == owner[e]) {
                                    ws.neg[slot * 64 + i * 8 + j] = -sqrtf(tot);
                                    ws.cost[slot * 64 + i * 8 + j] = cost_of_d2(tot);      // geomloss's cost from the same exact sum
                                }
                            }
                        }
                    }
                }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");   // scratch and stage buffers are reused by the next item
        __builtin_amdgcn_wave_barrier();
    }
}

// ---------------------------------------------------------------------------------------------
// Batch bounding-box diameter (geomloss max_diameter over the call's x and y tensors)
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kBlock) diameter_kernel(ScoreArgs a, int64_t group, int64_t ngroups, float* out) {
    __shared__ float part[kWaves];
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int dofs = threadIdx.x * 4;
    const bool paired = a.pairing == ASPIRE_PAIR_PAIRED;
    // CROSS: block = (query, group) folded into grid.x (grid.y stops at 65535 queries)
    const int64_t qy = paired ? 0 : (int64_t)(blockIdx.x / (uint32_t)ngroups);
    const int64_t g = paired ? (int64_t)blockIdx.x : (int64_t)blockIdx.x - qy * ngroups;
    const int64_t c_lo = g * group, c_hi = min(a.c.n, c_lo + group);
    float4 mn = make_float4(INFINITY, INFINITY, INFINITY, INFINITY);
    float4 mx = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
    auto add_rows = [&](const RepSet& s, int64_t k, bool use_ext) {
        const int n = (use_ext && s.ext > 0) ? s.ext : s.len[k];
        const float* doc = s.rows + (size_t)s.start[k] * kD;
        for (int r = 0; r < n; ++r) {
            const float4 v = ld4(doc + (size_t)r * kD + dofs);
            mn.x = fminf(mn.x, v.x); mn.y = fminf(mn.y, v.y); mn.z = fminf(mn.z, v.z); mn.w = fminf(mn.w, v.w);
            mx.x = fmaxf(mx.x, v.x); mx.y = fmaxf(mx.y, v.y); mx.z = fmaxf(mx.z, v.z); mx.w = fmaxf(mx.w, v.w);
        }
    };
    bool zero_row = false;
    if (paired) {
        for (int64_t k = c_lo; k < c_hi; ++k) {
            add_rows(a.q, k, true);
            add_rows(a.c, k, true);
        }
    } else {
        add_rows(a.q, qy, false);
        int lmin = 1 << 30, lmax = 0;
        for (int64_t k = c_lo; k < c_hi; ++k) {
            add_rows(a.c, k, false);
            lmin = min(lmin, a.c.len[k]);
            lmax = max(lmax, a.c.len[k]);
        }
        zero_row = lmin != lmax;  // caching_score zero-pads shorter candidates to the group max
    }
    if (zero_row) {
        mn.x = fminf(mn.x, 0.f); mn.y = fminf(mn.y, 0.f); mn.z = fminf(mn.z, 0.f); mn.w = fminf(mn.w, 0.f);
        mx.x = fmaxf(mx.x, 0.f); mx.y = fmaxf(mx.y, 0.f); mx.z = fmaxf(mx.z, 0.f); mx.w = fmaxf(mx.w, 0.f);
    }
    const float dx = mx.x - mn.x, dy = mx.y - mn.y, dz = mx.z - mn.z, dw = mx.w - mn.w;
    const float s = wave_sum(fmaf(dw, dw, fmaf(dz, dz, fmaf(dy, dy, dx * dx))));
    if (lane == 0) part[wave] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        out[blockIdx.x] = sqrtf(part[0] + part[1] + part[2]);
    }
}

}  // namespace

// ---------------------------------------------------------------------------------------------
// host side: the launchers (score_types.h)
// ---------------------------------------------------------------------------------------------
// max-sim on the VALU tiles: grid.x = candidates, grid.y = query chunks (a.q_per_block queries each; one-query pairings: 1)
int launch_l2max_tiles(const ScoreArgs& a, int max_rows, int qchunks, hipStream_t stream) {
    return dispatch_T(max_rows, [&](auto tc) -> int {
        constexpr int T = decltype(tc)::value;
        hipLaunchKernelGGL(l2max_kernel<T>, dim3((unsigned)a.c.n, (unsigned)qchunks, 1), dim3(kBlock), Lds<T>::kTotal * sizeof(float), stream, a);
        ASPIRE_LAUNCH_OK();
        return (int)ASPIRE_OK;
    });
}

// per-coordinate boxes of the documents of `d` -> box[d.n][2][768]
int launch_doc_box(const RepSet& d, float* box, hipStream_t stream) {
    hipLaunchKernelGGL(doc_box_kernel, dim3((unsigned)d.n), dim3(192), 0, stream, d, box);
    ASPIRE_LAUNCH_OK();
    return ASPIRE_OK;
}

// ---- stage 1 of an otAspire pass: pairwise costs of the chunk [a.cand0, a.cand1) -> workspace slots ---------------------
// (MAPPED pairing: the whole batch, or with `tile_blocks` > 0 the jobs [a.job0, a.job1) on the throughput kernel.)
int launch_cost_stage(const ScoreArgs& a, int T_rt, const aspire_repset* q, const aspire_repset* c, float* cost, float* neg, float* diam2,
                      int64_t n_slots, int qchunks, bool gram, float* qbox, float* cbox, bool first_chunk, hipStream_t stream) {
    // which kernel: forms.hip
    const CostChoice ch = cost_kernel_form(T_rt, q, c, a.pairing, gram, a.tile_form != 0, a.grp_off != nullptr, a.cand1 - a.cand0,
                                           a.job1 - a.job0, a.max_job_groups, n_slots);
    if (ch.kernel == CostKernel::Gram)
        return launch_pair_gram_ot(a, T_rt, q->max_len, c->max_len, cost, neg, a.diameter ? nullptr : diam2, qbox, cbox, stream);
    // the streaming kernels take the per-coordinate boxes of the queries, once per call (MAPPED: the tables launch wrote them)
    if ((ch.kernel == CostKernel::Tile || ch.kernel == CostKernel::Tile16) && !a.diameter && first_chunk && a.pairing != kPairMapped)
        if (int rc = launch_doc_box(a.q, qbox, stream)) return rc;
    if (ch.kernel == CostKernel::Tile16) return launch_pair_tile16(a, cost, neg, diam2, ch.items, qbox, stream);
    return dispatch_T(8 * T_rt, [&](auto tc) -> int {
        constexpr int T = decltype(tc)::value;
        const PairWs<T> ws{cost, neg, diam2};
        const PairWs<1> ws1{cost, neg, diam2};
        const bool csr = q->ext == 0 && c->ext == 0;
        if (ch.kernel == CostKernel::Tile) {
            const int64_t wave_cap = tuning().tile_waves > 0 ? tuning().tile_waves : 256 * 8;      // TILE_WAVES: tests with several items per wave
            const int64_t waves = ch.items < wave_cap ? ch.items : wave_cap;
            hipLaunchKernelGGL(pair_tile_kernel, dim3((unsigned)((waves + 3) / 4)), dim3(256),
                               4 * TileCfg::kLdsFloats * sizeof(float), stream, a, ws1, qbox);
        } else if (ch.kernel == CostKernel::Cost1) {
            // One pair per workgroup up to 2048 pairs (at ~1000 pairs it beats 512 persistent workgroups with two each, alone
            // and beside other launches); beyond, 512 persistent workgroups = what is resident at two per CU.
            const int cap_t = tuning().cost1_blocks;
            const int64_t cap = cap_t > 0 ? cap_t : (n_slots <= 2048 ? 2048 : 512);
            const int64_t blocks = n_slots < cap ? n_slots : cap;
            hipLaunchKernelGGL(pair_cost1_kernel, dim3((unsigned)blocks), dim3(kBlock), Lds<1>::kTotal * sizeof(float), stream, a,
                               ws1, 1u);
        } else if (ch.kernel == CostKernel::Cost1Sub) {
            hipLaunchKernelGGL(pair_cost1_sub_kernel, dim3((unsigned)(ch.items < 1024 ? ch.items : 1024)), dim3(kBlock),
                               Lds<1>::kTotal * sizeof(float), stream, a, ws1, (uint32_t)T);
        } else if (csr && a.center) {        // rows with a large common component: the same kernel on centred rows
            hipLaunchKernelGGL((pair_cost_kernel<T, false, true>), dim3((unsigned)(a.cand1 - a.cand0), (unsigned)qchunks, 1), dim3(kBlock),
                               Lds<T>::kTotal * sizeof(float), stream, a, ws);
        } else if (csr) {
            hipLaunchKernelGGL((pair_cost_kernel<T, false>), dim3((unsigned)(a.cand1 - a.cand0), (unsigned)qchunks, 1), dim3(kBlock),
                               Lds<T>::kTotal * sizeof(float), stream, a, ws);
        } else {
            hipLaunchKernelGGL((pair_cost_kernel<T, true>), dim3((unsigned)(a.cand1 - a.cand0), (unsigned)qchunks, 1), dim3(kBlock),
                               Lds<T>::kTotal * sizeof(float), stream, a, ws);
        }
        ASPIRE_LAUNCH_OK();
        return (int)ASPIRE_OK;
    });
}

// The hybrid forms' gate (ScoreArgs::gate): a census of the long pairs on the device, and the limit the queued kernels compare it to --
// up to ~4 % long pairs (measured crossover at 20 x 1000: 5 %): fused kernel + the 16-row kernels on the long pairs only.
int arm_long_pair_gate(ScoreArgs& a, int32_t* gate, int64_t C, hipStream_t s) {
    ASPIRE_HIP_OK(hipMemsetAsync(gate, 0, sizeof(int32_t), s));
    hipLaunchKernelGGL(long_pair_census_kernel, dim3((unsigned)((C + 255) / 256)), dim3(256), 0, s, a, gate);
    ASPIRE_LAUNCH_OK();
    a.gate = gate;
    a.gate_limit = (int32_t)(C / 24);
    return ASPIRE_OK;
}

// one box diameter per block: `blocks` = groups (PAIRED) or (query, group) folded into grid.x (CROSS)
int launch_group_diameter(const ScoreArgs& a, int64_t group, int64_t ngroups, int64_t blocks, float* diameter, hipStream_t stream) {
    hipLaunchKernelGGL(diameter_kernel, dim3((unsigned)blocks), dim3(kBlock), 0, stream, a, group, ngroups, diameter);
    ASPIRE_LAUNCH_OK();
    return ASPIRE_OK;
}

}  // namespace aspire
