// The rule for an L2 entry whose expansion cancels, and the exact sums that serve it (device only; include after common.h).
//
// Every kernel family forms d^2 = |x|^2 - 2 x.y + |y|^2 and keeps only x.y per entry.  Where that cancels -- two (nearly) equal
// sentence rows -- the fp32 expansion is rounding noise of |x|^2, so the entry is redone from the exact sum of squared
// differences, and BOTH -cdist and geomloss's cost come from that sum (include/aspire_hip.h, SHARED SENTENCES).
// (round 6: a cancelling entry is redone from the exact sum whatever formula torch.cdist would pick -- also beyond 25 rows: include/aspire_hip.h, SHARED SENTENCES)
//
// The exact sum has three forms, by who is free to walk the two rows; each keeps its own order of summation:
//   A  the whole wave on one entry: 12 coordinates per lane in one chain, then wave_sum; redo_wave4 takes four entries per memory
//      round trip (fused_kernel_body.h, tile16.hip; cost_valu.hip's pair_tile_kernel keeps its own loop around wave_d2_part, which
//      costs it two registers fewer: NOTES.md; sinkhorn.hip's pair_one_kernel takes one entry at a time)
//   B  16 lanes (one DPP row) on one entry: 48 coordinates per lane in two chains (gram.hip, gramp.hip, cost_valu.hip's pair_cost1_body)
//   C  one lane walks both rows: two chains of 4 over 8 coordinates a step (gram.hip's direct_d2, cost_valu.hip's lane-local redos;
//      l2agg_pair.hip's exact_d2 is the same sum with its loop kept rolled)
// Forms B and C take the rows' 16-byte loads as functors of the float offset: gram.hip reads through global-address-space
// pointers and gramp.hip by row index, and neither may become a flat load.
#pragma once

namespace aspire {

constexpr float kCancelTau = 1e-4f;      // the expansion cancels where d^2 < tau (|x|^2 + |y|^2)^2
constexpr float kCostFloor2 = 1e-8f;     // geomloss's clamp_min on the squared distance

// sq = the expansion, ns = |x|^2 + |y|^2
__device__ __forceinline__ bool expansion_cancels(float sq, float ns) { return sq < kCancelTau * ns * ns; }
__device__ __forceinline__ float cost_of_d2(float d2) { return sqrtf(fmaxf(d2, kCostFloor2)); }
__device__ __forceinline__ float neg_of_expansion(float sq) { return -sqrtf(fmaxf(sq, 0.f)); }
// the same cost from a distance that is already a square root (= sqrt(max(d^2, kCostFloor2)))
__device__ __forceinline__ float cost_of_dist(float d) { return fmaxf(d, __builtin_sqrtf(kCostFloor2)); }

// one step of a chain: s + the four squared differences, in this order
__device__ __forceinline__ float sq_chain4(float d0, float d1, float d2, float d3, float s) {
    return fmaf(d3, d3, fmaf(d2, d2, fmaf(d1, d1, fmaf(d0, d0, s))));
}
template <class V>
__device__ __forceinline__ float d2_step(const V& u, const V& v, float s) {
    return sq_chain4(u.x - v.x, u.y - v.y, u.z - v.z, u.w - v.w, s);
}
// two independent chains side by side (forms B and C): the eight differences, then the two chains
template <class V>
__device__ __forceinline__ void d2_step2(const V& u0, const V& v0, const V& u1, const V& v1, float& s0, float& s1) {
    const float a0 = u0.x - v0.x, a1 = u0.y - v0.y, a2 = u0.z - v0.z, a3 = u0.w - v0.w;
    const float b0 = u1.x - v1.x, b1 = u1.y - v1.y, b2 = u1.z - v1.z, b3 = u1.w - v1.w;
    s0 = sq_chain4(a0, a1, a2, a3, s0);
    s1 = sq_chain4(b0, b1, b2, b3, s1);
}

struct RowPair { const float *x, *y; };

// ---- form A: a lane's 12 coordinates (floats 4 lane + 256 t of the two rows); the entry is wave_sum of it ----
template <class V>
__device__ __forceinline__ float wave_d2_part(const V (&u)[3], const V (&v)[3]) {
    float part = 0.f;
#pragma unroll
    for (int t = 0; t < 3; ++t) part = d2_step(u[t], v[t], part);
    return part;
}

// The flagged lanes of `wm` (a ballot), FOUR entries per memory round trip: all 24 loads go out before the first is consumed, with
// no branch around them (an empty slot repeats the first entry's rows).  Under a saturated HBM stream a dependent round trip
// is ~5 us, and a wave that falls behind by n of them finishes the launch n x 5 us late (one duplicate document = 8 entries in a
// 20 000-pair call, one entry per round trip: 145 instead of 101 us).
// rows(o): the two rows of owner lane o's entry as a RowPair, wave-uniform; store(o, d2): runs in the owner lane alone.
template <class Rows, class Store>
__device__ __forceinline__ void redo_wave4(unsigned long long wm, int lane, Rows&& rows, Store&& store) {
    while (wm != 0) {
        int owner[4];
        float part[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            owner[e] = wm != 0 ? (int)__builtin_ctzll(wm) : -1;
            wm = wm != 0 ? wm & (wm - 1) : 0;
        }
        float4 u[4][3], v[4][3];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const RowPair r = rows(owner[e] >= 0 ? owner[e] : owner[0]);
#pragma unroll
            for (int t = 0; t < 3; ++t) {
                u[e][t] = *reinterpret_cast<const float4*>(r.x + 4 * lane + 256 * t);
                v[e][t] = *reinterpret_cast<const float4*>(r.y + 4 * lane + 256 * t);
            }
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) part[e] = wave_d2_part(u[e], v[e]);
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (owner[e] >= 0) {
                const float tot = wave_sum(part[e]);
                if (lane == owner[e]) store(owner[e], tot);
            }
    }
}

// ---- form B: the entry's sum in each of the 16 lanes of a DPP row; lane l16 takes floats 4 l16 + 64 c, c = 0 .. 11 (the
// functors add the lane's 4 l16) ----
template <class LdX, class LdY>
__device__ __forceinline__ float row16_d2(LdX&& ldx, LdY&& ldy) {
    float p0 = 0.f, p1 = 0.f;
#pragma unroll
    for (int c = 0; c < 12; c += 2) {
        const auto u0 = ldx(64 * c), v0 = ldy(64 * c);
        const auto u1 = ldx(64 * c + 64), v1 = ldy(64 * c + 64);
        d2_step2(u0, v0, u1, v1, p0, p1);
    }
    float part = p0 + p1;
    part += lane_xor<1>(part);
    part += lane_xor<2>(part);
    part += lane_xor<4>(part);
    part += lane_xor<8>(part);
    return part;
}

// ---- form C: one lane walks the 768 coordinates of both rows ----
template <class LdX, class LdY>
__device__ __forceinline__ float lane_d2(LdX&& ldx, LdY&& ldy) {
    float s0 = 0.f, s1 = 0.f;
    for (int k = 0; k < kD; k += 8) {
        const auto a = ldx(k), b = ldy(k), c = ldx(k + 4), d = ldy(k + 4);
        d2_step2(a, b, c, d, s0, s1);
    }
    return s0 + s1;
}

}  // namespace aspire
