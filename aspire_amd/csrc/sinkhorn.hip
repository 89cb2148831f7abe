// The Sinkhorn solvers of the otAspire path on workspace slots: soft-max marginals (A6) and geomloss-0.2.4's annealed solve
// (A7/A8), one solve per wave (sinkhorn_kernel, sinkhorn_repair_kernel), many per wave (sinkhorn_block_kernel), and the one-launch
// form that forms a short pair's costs in the wave that solves it (pair_one_kernel).  Reference arithmetic:
//   src/learning/facetid_models/pair_distances.py:57-92 (allenai/aspire)
//   geomloss==0.2.4 sinkhorn_tensorized / sinkhorn_loop (third party; restated, parity unpinned).
//
// The solve of one (query, candidate) pair runs in ONE wave with lane (li,lj) = (l>>3,l&7) holding the T x T entries
// (8a+li, 8b+lj): row log-sum-exps are DPP reductions over lane bits 0-2, column ones over bits 3-5 (permlane swaps);
// potentials stay in registers for all ~70 eps-steps.  sinkhorn_pair is not __forceinline__ and the compiler inlines it into each of
// its callers (sinkhorn_kernel, pair_one_kernel, sinkhorn_repair_kernel): all of them are defined in this file, so that it weighs
// the same set of call sites whichever of them changes.
//
// Host side (the end of the file): launch_sinkhorn_stage picks the solver form of a launch, launch_pair_one starts the
// one-launch form; both are declared in score_types.h.
#include <math.h>

#include <type_traits>

#include "common.h"
#include "tuning.h"
#include "forms.h"
#include "score_types.h"
#include "score_device.h"
#include "exact_d2.h"

namespace aspire {
namespace {

// ---------------------------------------------------------------------------------------------
// otAspire kernel (A5-A8)
// ---------------------------------------------------------------------------------------------
template <int T>
struct PairState {
    float cost[T][T];  // geomloss cost: sqrt(max(|x|^2 - 2 x.y + |y|^2, 1e-8))
    float neg[T][T];   // -cdist (torch formula)
};

// Lane <-> entry map of the one-solve-per-wave kernel.  T > 1: (li, lj) = (lane >> 3, lane & 7).  T == 1 spreads the
// two cross-row lane bits over BOTH index directions -- lj = lane bits {0, 1, 4}, li = lane bits {2, 3, 5} -- so that
// each of the two reductions of a Sinkhorn step is two DPP levels plus ONE v_permlane*_swap, instead of three DPP
// levels for the rows and one DPP level plus two swaps (mov + swap + add each, the longest links of the dependent
// chain) for the columns.
template <int T>
__device__ __forceinline__ void lane_ij(int lane, int& li, int& lj) {
    if constexpr (T == 1) {
        lj = (lane & 3) | ((lane >> 2) & 4);
        li = ((lane >> 2) & 3) | ((lane >> 3) & 4);
    } else {
        li = lane >> 3;
        lj = lane & 7;
    }
}
template <int T>
__device__ __forceinline__ float rsum8(float v) {   // all-reduce over the 8 lanes that share li
    if constexpr (T == 1) {
        v += lane_xor<1>(v);
        v += lane_xor<2>(v);
        return swap_add<16>(v, v);
    } else {
        return row8_sum(v);
    }
}
template <int T>
__device__ __forceinline__ float csum8(float v) {   // all-reduce over the 8 lanes that share lj
    if constexpr (T == 1) {
        v += dpp_mov<0x124>(v, v);   // row_ror:4
        v += dpp_mov<0x128>(v, v);   // row_ror:8
        return swap_add<32>(v, v);
    } else {
        return col8_sum(v);
    }
}
template <int T>
__device__ __forceinline__ float rmax8(float v) {
    if constexpr (T == 1) {
        v = fmaxf(v, lane_xor<1>(v));
        v = fmaxf(v, lane_xor<2>(v));
        return fmaxf(v, lane_xor<16>(v));
    } else {
        return row8_max(v);
    }
}
template <int T>
__device__ __forceinline__ float cmax8(float v) {
    if constexpr (T == 1) {
        v = fmaxf(v, dpp_mov<0x124>(v, v));
        v = fmaxf(v, dpp_mov<0x128>(v, v));
        return fmaxf(v, lane_xor<32>(v));
    } else {
        return col8_max(v);
    }
}

template <int T>
__device__ __forceinline__ void load_pair(PairState<T>& s, const PairWs<T>& ws, int64_t slot, int lane, bool cost_from_neg = false) {
    int li, lj;
    lane_ij<T>(lane, li, lj);
#pragma unroll
    for (int ta = 0; ta < T; ++ta)
#pragma unroll
        for (int tb = 0; tb < T; ++tb) {
            const int64_t o = slot * (64 * T * T) + (ta * 8 + li) * (8 * T) + tb * 8 + lj;
            s.neg[ta][tb] = ws.neg[o];
            // (the matrix-pipe cost tiles store -cdist only: sqrt(max(sq, 1e-8)) = max(sqrt(max(sq, 0)), sqrt(1e-8)) bit for bit)
            s.cost[ta][tb] = cost_from_neg ? cost_of_dist(-s.neg[ta][tb]) : ws.cost[o];
        }
}

template <int T>
__device__ void sinkhorn_pair(const ScoreArgs& a, const PairState<T>& s, int q_len, int c_len, float diam, int64_t p,
                              int lane) {
    int li, lj;
    lane_ij<T>(lane, li, lj);
    bool rv[T], cv[T];  // row / column validity
#pragma unroll
    for (int t = 0; t < T; ++t) {
        rv[t] = t * 8 + li < q_len;
        cv[t] = t * 8 + lj < c_len;
    }
    // ---- marginals (pair_distances.py:57-60): softmax over sentences of the best match / temp -----
    const float temp = (float)a.temp;
    float la[T], lb[T], wa[T], wb[T];  // log-weights and weights
    {
        float qm[T], cm[T];
#pragma unroll
        for (int ta = 0; ta < T; ++ta) {
            float m = kNegBig;
#pragma unroll
            for (int tb = 0; tb < T; ++tb) m = fmaxf(m, (rv[ta] && cv[tb]) ? s.neg[ta][tb] : kNegBig);
            qm[ta] = rmax8<T>(m) / temp;
        }
#pragma unroll
        for (int tb = 0; tb < T; ++tb) {
            float m = kNegBig;
#pragma unroll
            for (int ta = 0; ta < T; ++ta) m = fmaxf(m, (rv[ta] && cv[tb]) ? s.neg[ta][tb] : kNegBig);
            cm[tb] = cmax8<T>(m) / temp;
        }
        float mq = kNegBig, mc = kNegBig;
#pragma unroll
        for (int t = 0; t < T; ++t) {
            mq = fmaxf(mq, rv[t] ? qm[t] : kNegBig);
            mc = fmaxf(mc, cv[t] ? cm[t] : kNegBig);
        }
        mq = cmax8<T>(mq);  // rows are spread over lane bits 3-5
        mc = rmax8<T>(mc);  // columns over lane bits 0-2
        float sq = 0.f, sc = 0.f;
#pragma unroll
        for (int t = 0; t < T; ++t) {
            sq += rv[t] ? fast_exp(qm[t] - mq) : 0.f;
            sc += cv[t] ? fast_exp(cm[t] - mc) : 0.f;
        }
        const float lsq = fast_log(csum8<T>(sq)), lsc = fast_log(rsum8<T>(sc));
#pragma unroll
        for (int t = 0; t < T; ++t) {
            // log_softmax(...).exp(), then geomloss log_weights: log(a), a <= 0 -> -100000
            wa[t] = rv[t] ? fast_exp(qm[t] - mq - lsq) : 0.f;
            wb[t] = cv[t] ? fast_exp(cm[t] - mc - lsc) : 0.f;
            la[t] = wa[t] > 0.f ? fast_log(wa[t]) : -100000.f;
            lb[t] = wb[t] > 0.f ? fast_log(wb[t]) : -100000.f;
        }
    }
    // ---- epsilon schedule (geomloss epsilon_schedule, p = 1) --------------------------------------
    //   [diam] + [exp(e) for e in arange(log diam, log blur, log scaling)] + [blur]
    float ldf;                                    // log2 units
    const int n_mid = schedule_mid_steps(a, diam, ldf);
    const float lscf = a.log2_scaling;
    const float eps_last = (float)a.blur;

    float f[T], g[T];
    // out_i = -eps * logsumexp_j(hb_j - C_ij/eps) over valid j   (rows; `shift` = the caller's estimate of
    // -logsumexp, see step()).  With EXACT the shift is the true maximum, as torch.logsumexp does.
    auto lse_rows = [&](float eps, const float (&qc)[T][T], const float (&h)[T], const float (&shift)[T], bool exact,
                        float (&out)[T]) {
#pragma unroll
        for (int ta = 0; ta < T; ++ta) {
            float tv[T];
#pragma unroll
            for (int tb = 0; tb < T; ++tb) tv[tb] = cv[tb] ? h[tb] - qc[ta][tb] : kNegBig;
            float m = -shift[ta];
            if (exact) {
                m = tv[0];
#pragma unroll
                for (int tb = 1; tb < T; ++tb) m = fmaxf(m, tv[tb]);
                m = rmax8<T>(m);
            }
            float sum = 0.f;
#pragma unroll
            for (int tb = 0; tb < T; ++tb) sum += fast_exp(tv[tb] - m);
            out[ta] = -eps * (m + fast_log(rsum8<T>(sum)));
        }
    };
    auto lse_cols = [&](float eps, const float (&qc)[T][T], const float (&h)[T], const float (&shift)[T], bool exact,
                        float (&out)[T]) {
#pragma unroll
        for (int tb = 0; tb < T; ++tb) {
            float tv[T];
#pragma unroll
            for (int ta = 0; ta < T; ++ta) tv[ta] = rv[ta] ? h[ta] - qc[ta][tb] : kNegBig;
            float m = -shift[tb];
            if (exact) {
                m = tv[0];
#pragma unroll
                for (int ta = 1; ta < T; ++ta) m = fmaxf(m, tv[ta]);
                m = cmax8<T>(m);
            }
            float sum = 0.f;
#pragma unroll
            for (int ta = 0; ta < T; ++ta) sum += fast_exp(tv[ta] - m);
            out[tb] = -eps * (m + fast_log(csum8<T>(sum)));
        }
    };
    // One symmetric Sinkhorn update at `eps` (reps = 1/eps):
    //   gt_j = -eps*LSE_i(la_i + f_i/eps - C_ij/eps),  ft_i = -eps*LSE_j(lb_j + g_j/eps - C_ij/eps)
    // The log-sum-exps are stabilised by shifting with -g_j/eps resp. -f_i/eps -- the previous
    // potentials, which ARE (-eps times) the previous log-sum-exps -- instead of the running maximum:
    // mathematically identical, the sum then sits near 1, and six dependent cross-lane max steps leave
    // the critical path.  If a sum ever leaves [1e-30, 1e30] (it cannot while potentials move by less
    // than ~69*eps per step) the step is redone with the exact maximum.
    auto step = [&](float eps, float reps, bool averaged, bool exact) {
        float qc[T][T], qf[T], qg[T], ha[T], hb[T], ft[T], gt[T];
#pragma unroll
        for (int ta = 0; ta < T; ++ta)
#pragma unroll
            for (int tb = 0; tb < T; ++tb) qc[ta][tb] = div_r(s.cost[ta][tb], eps, reps);
#pragma unroll
        for (int t = 0; t < T; ++t) {
            qf[t] = div_r(f[t], eps, reps);
            qg[t] = div_r(g[t], eps, reps);
            ha[t] = la[t] + qf[t];
            hb[t] = lb[t] + qg[t];
        }
        lse_cols(eps, qc, ha, qg, exact, gt);
        lse_rows(eps, qc, hb, qf, exact, ft);
#pragma unroll
        for (int t = 0; t < T; ++t) {
            g[t] = averaged ? 0.5f * (g[t] + gt[t]) : gt[t];
            f[t] = averaged ? 0.5f * (f[t] + ft[t]) : ft[t];
        }
    };
    // The same update with the critical path cut to the bone (the kernel's time at ~1000 pairs IS 75 x this
    // chain).  Everything is in base 2 (r2 = log2(e)/eps, rounded once from float64, so v_exp_f32 / v_log_f32 need no
    // scaling multiplies) and the state carried from step to step is phi_ij = f_i + g_j - C_ij itself:
    //     sum_j b_j 2^(phi_ij r2) = exp((f_i - ft_i)/eps)        sum_i a_i 2^(phi_ij r2) = exp((g_j - gt_j)/eps)
    // (the log-sum-exps shifted by the previous potentials), so with LR_i, LC_j the log2 of those sums the averaged
    // update is  f_i -= h LR_i,  g_j -= h LC_j,  phi_ij -= h (LR_i + LC_j),  h = eps ln2 / 2  (eps ln2 for the final
    // extrapolation).  The dependent chain per step is fma - exp2 - reduce - log2 - add - fma; f and g are updated
    // off that chain.  phi's rounding matters only where |phi| is small (the transport plan's support), where its
    // ulp is far below the tolerance.  Measured against a float64 evaluation this is as accurate as the fp32 CPU
    // path (tools/oterr.py).
    float la2[T], lb2[T];
#pragma unroll
    for (int t = 0; t < T; ++t) {
        la2[t] = la[t] * kLog2e;
        lb2[t] = lb[t] * kLog2e;
    }
    float phi[T][T];
    auto phi_init = [&]() {
#pragma unroll
        for (int ta = 0; ta < T; ++ta)
#pragma unroll
            for (int tb = 0; tb < T; ++tb)
                phi[ta][tb] = (rv[ta] && cv[tb]) ? (f[ta] + g[tb]) - s.cost[ta][tb] : -__builtin_inff();   // masked slots may hold stale bits
    };
    float pad1[T][T];
#pragma unroll
    for (int ta = 0; ta < T; ++ta)
#pragma unroll
        for (int tb = 0; tb < T; ++tb) pad1[ta][tb] = (rv[ta] && cv[tb]) ? 0.f : 1.f;
    // One exponential per entry and no potentials in the loop: E_ij = 2^(phi_ij r2) serves both sums with the marginal
    // weights as plain factors (sum_j b_j E_ij, sum_i a_i E_ij), and since sum a = sum b = 1 the result
    //     <a, f> + <b, g> = sum_ij a_i b_j (f_i + g_j) = sum_ij a_i b_j (phi_ij + C_ij)
    // needs phi alone -- f and g are never formed on this path.  With one entry per lane (T == 1) the update
    // h (LR_i + LC_j) = h log2(rowsum_i * colsum_j) is ONE logarithm: two transcendentals per entry and step instead
    // of four (they issue at quarter rate: the lone launch's dependent chain is unchanged, but overlapped queries share
    // the SIMDs' issue slots -- bench.py 110 -> 115 M alignments/s; 1 x 125 x 20 35.6 -> 31.4 us).  Masked entries carry phi = -inf (E = 0, out of every sum)
    // and a +1 on their own (empty) sums keeps their logarithm at 0.
    // A step at temperature eps:  E = 2^(phi r2),  phi -= h log2(rowsum colsum),  r2 = log2(e)/eps,  h = eps ln2 / 2
    // (eps ln2 for the final, un-averaged step).  Through the geometric part of the schedule the constants of the next
    // step follow from this one's by the factor scaling (r2 /= scaling, h *= scaling): two multiplies off the dependent
    // chain instead of two v_readlane broadcasts of a per-lane table, and nothing for the loop to index, so it
    // unrolls freely.  (Carrying psi = phi r2 instead saves one more multiply per step but rescales the state 77 times:
    // mean error against float64 8.6e-6 instead of 5.4e-6.)
    float r2v = 0.f, hv = 0.f;       // wave-uniform, kept in vector registers: gfx950 has no scalar float multiply
    auto step2 = [&](float r2_mul, float h_mul) {
        if constexpr (T == 1) {
            // One entry per lane.  The column chain and the row chain (two DPP levels and one v_permlane*_swap each,
            // see lane_ij) are independent; a single wave issues in order, so they are interleaved level by level
            // here and pinned with sched_barrier -- a cross-lane op costs 17-26 cycles of dependent latency
            // (tools: build/dbg/lat.hip), overlapped they cost it once, not twice.
            const float e = __builtin_amdgcn_exp2f(phi[0][0] * r2v);
            float sc = wa[0] * e;
            float sr = wb[0] * e;
            // opaque to the optimizer: left alone it contracts a * b + dpp(a * b) into mov_dpp + fma, two issue slots
            // per step more than mul + add_dpp
            asm volatile("" : "+v"(sc), "+v"(sr));
            __builtin_amdgcn_sched_barrier(0);
            sc += dpp_mov<0x124>(sc, sc);     // columns: lane bits 2, 3 (row_ror:4, row_ror:8), then bit 5
            sr += lane_xor<1>(sr);            // rows:    lane bits 0, 1 (quad_perm), then bit 4
            __builtin_amdgcn_sched_barrier(0);
            sc += dpp_mov<0x128>(sc, sc);
            sr += lane_xor<2>(sr);
            __builtin_amdgcn_sched_barrier(0);
            sc = swap_add<32>(sc, sc);
            sr = swap_add<16>(sr, sr);
            __builtin_amdgcn_sched_barrier(0);
            phi[0][0] = fmaf(-hv, __builtin_amdgcn_logf(fmaf(sc, sr, pad1[0][0])), phi[0][0]);
        } else {
            float e[T][T], lr[T], lc[T];
#pragma unroll
            for (int ta = 0; ta < T; ++ta)
#pragma unroll
                for (int tb = 0; tb < T; ++tb) e[ta][tb] = __builtin_amdgcn_exp2f(phi[ta][tb] * r2v);
#pragma unroll
            for (int tb = 0; tb < T; ++tb) {   // columns
                float sum = 0.f;
#pragma unroll
                for (int ta = 0; ta < T; ++ta) sum = fmaf(wa[ta], e[ta][tb], sum);
                lc[tb] = __builtin_amdgcn_logf(csum8<T>(sum) + (cv[tb] ? 0.f : 1.f));
            }
#pragma unroll
            for (int ta = 0; ta < T; ++ta) {   // rows
                float sum = 0.f;
#pragma unroll
                for (int tb = 0; tb < T; ++tb) sum = fmaf(wb[tb], e[ta][tb], sum);
                lr[ta] = __builtin_amdgcn_logf(rsum8<T>(sum) + (rv[ta] ? 0.f : 1.f));
            }
#pragma unroll
            for (int ta = 0; ta < T; ++ta)
#pragma unroll
                for (int tb = 0; tb < T; ++tb) phi[ta][tb] = fmaf(-hv, lr[ta] + lc[tb], phi[ta][tb]);
        }
        r2v *= r2_mul;      // the next step's constants
        hv *= h_mul;
    };
    // The whole annealing loop.  exact = false uses the shifted log-sum-exp; an overflowed / vanished
    // sum turns into inf / nan that then sticks to the potentials, so ONE finiteness test at the end
    // (instead of a compare + branch on every step's critical path) decides whether the solve has to be
    // repeated with exact maxima.
    auto solve = [&](bool exact) {
        if (exact) {   // initialisation at eps_s[0] = diam: softmin of the bare log-weights, exact maximum
            const float reps = rcp_refined(diam);
            float qc[T][T], zero[T];
#pragma unroll
            for (int ta = 0; ta < T; ++ta)
#pragma unroll
                for (int tb = 0; tb < T; ++tb) qc[ta][tb] = div_r(s.cost[ta][tb], diam, reps);
#pragma unroll
            for (int t = 0; t < T; ++t) zero[t] = 0.f;
            lse_cols(diam, qc, la, zero, true, g);
            lse_rows(diam, qc, lb, zero, true, f);
            step(diam, reps, true, true);
        } else {
            // the same initialisation without a max shift (the largest weight of a probability vector over <= 32
            // atoms is >= 1/32 and C/diam <= ~1, so the sums stay in range), weights as plain factors, then the
            // first averaged step at eps = diam in the phi form like all the others
            const float r2d = kLog2e * rcp_refined(diam), eln2d = diam * kLn2;
            float rs[T], cs[T];
#pragma unroll
            for (int t = 0; t < T; ++t) rs[t] = cs[t] = 0.f;
#pragma unroll
            for (int ta = 0; ta < T; ++ta)
#pragma unroll
                for (int tb = 0; tb < T; ++tb) {
                    const float k0 = (rv[ta] && cv[tb]) ? __builtin_amdgcn_exp2f(-s.cost[ta][tb] * r2d) : 0.f;
                    rs[ta] = fmaf(wb[tb], k0, rs[ta]);
                    cs[tb] = fmaf(wa[ta], k0, cs[tb]);
                }
#pragma unroll
            for (int t = 0; t < T; ++t) {
                f[t] = -eln2d * __builtin_amdgcn_logf(rsum8<T>(rs[t]));
                g[t] = -eln2d * __builtin_amdgcn_logf(csum8<T>(cs[t]));
            }
            phi_init();
            // steps: eps = diam, then the n_mid annealed values diam scaling^k (k = 0 .. n_mid - 1; fp32 -- a relative
            // 1e-6 on an intermediate temperature moves the result by far less than the tolerance, and the float64 exp
            // cost as much as ten annealing steps), then blur, then the final un-averaged step at blur
            const float rho_s = __builtin_amdgcn_exp2f(-lscf), scal = __builtin_amdgcn_exp2f(lscf);     // 1 / scaling, scaling
            const float last_eps = n_mid > 0 ? __builtin_amdgcn_exp2f(fmaf((float)(n_mid - 1), lscf, ldf)) : diam;
            const float rho_b = last_eps * rcp_refined(eps_last), inv_rho_b = eps_last * rcp_refined(last_eps);
            const int n_s = __builtin_amdgcn_readfirstlane(n_mid);                          // wave-uniform: scalar loop control
            r2v = r2d;
            hv = 0.5f * eln2d;
            step2(n_s > 0 ? 1.f : rho_b, n_s > 0 ? 1.f : inv_rho_b);                        // at diam
            int k = 1;
            for (; k + 4 <= n_s; k += 4) {      // unrolled by hand (the pinned schedule inside step2 defeats #pragma unroll)
                step2(rho_s, scal);
                step2(rho_s, scal);
                step2(rho_s, scal);
                step2(rho_s, scal);
            }
            for (; k < n_s; ++k) step2(rho_s, scal);
            if (n_s > 0) step2(rho_b, inv_rho_b);                                            // the last annealed value -> blur
            // the two steps at blur with exactly rounded constants (drops the drift of the running products)
            r2v = kLog2e * rcp_refined(eps_last);
            hv = 0.5f * eps_last * kLn2;
            step2(1.f, 2.f);                                                                 // at blur, averaged
            step2(1.f, 1.f);                                                                 // at blur, final (h doubled)
            return;
        }

        // exact path only from here: float64 schedule exactly as numpy builds geomloss's, lane k of a chunk evaluates
        // eps_{base+k} and the per-step constants are broadcast with v_readlane
        const double ld = log((double)diam);
        for (int base = 0; base < n_mid; base += 64) {
            const float my_eps = (float)exp(ld + (double)(base + lane) * a.log_scaling);
            const float my_reps = rcp_refined(my_eps);
            const int cnt = min(64, n_mid - base);
            for (int k = 0; k < cnt; ++k) {
                const float eps = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, my_eps), k));
                const float reps = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, my_reps), k));
                step(eps, reps, true, true);
            }
        }
        const float rb = rcp_refined(eps_last);
        step(eps_last, rb, true, true);
        step(eps_last, rb, false, true);  // last extrapolation: simultaneous, not averaged
    };
    bool phi_live = true;
    solve(false);
    // <a, f> + <b, g> from phi alone (see step2); an overflowed / vanished sum anywhere has turned into inf / nan that
    // reaches this total, so its finiteness is the one test that decides whether the solve is repeated exactly.
    float fast_total;
    {
        float acc = 0.f;
#pragma unroll
        for (int ta = 0; ta < T; ++ta)
#pragma unroll
            for (int tb = 0; tb < T; ++tb)
                acc += (rv[ta] && cv[tb]) ? (wa[ta] * wb[tb]) * (phi[ta][tb] + s.cost[ta][tb]) : 0.f;
        fast_total = wave_sum(acc);
        if (__builtin_expect(!(fabsf(fast_total) < 1e30f), 0)) {
            solve(true);
            phi_live = false;
        }
    }
    const float rb = rcp_refined(eps_last);

    // ---- outputs ------------------------------------------------------------------------------
    float score;
    if (a.want != ASPIRE_OT_PLAN_SIM) {
        if (phi_live) {
            score = fast_total;
        } else {
            float acc = 0.f;
#pragma unroll
            for (int t = 0; t < T; ++t) {
                acc += (lj == 0 && rv[t]) ? wa[t] * f[t] : 0.f;
                acc += (li == 0 && cv[t]) ? wb[t] * g[t] : 0.f;
            }
            score = wave_sum(acc);
        }
        if (a.want == ASPIRE_OT_SIMILARITY) score = -score;
    } else {
        score = 0.f;
    }
    const bool dump = a.out_plan != nullptr || a.out_pairsims != nullptr;
    if (a.want == ASPIRE_OT_PLAN_SIM || dump) {
        float acc = 0.f;
#pragma unroll
        for (int ta = 0; ta < T; ++ta)
#pragma unroll
            for (int tb = 0; tb < T; ++tb) {
                const bool valid = rv[ta] && cv[tb];
                const float negm = valid ? s.neg[ta][tb] : 0.f;
                // f_i + g_j - dist_ij: after the fast solve phi = f + g - C is at hand with the rounding of ITS
                // magnitude (small on the plan's support) rather than of f's and g's, and C - dist is an exact
                // difference of two nearby floats -- eps = 0.05 amplifies this exponent's error ~20x.
                const float expo = !valid ? 0.f : phi_live ? phi[ta][tb] + (s.cost[ta][tb] + negm) : (f[ta] + g[tb]) + negm;
                const float plan = fast_exp(div_r(expo, eps_last, rb)) * (wa[ta] * wb[tb]);
                acc += plan * negm;
                const int i = ta * 8 + li, j = tb * 8 + lj;
                if (dump && i < a.q.ext && j < a.c.ext) {
                    const int64_t o = (p * a.q.ext + i) * a.c.ext + j;
                    if (a.out_plan) a.out_plan[o] = plan;
                    if (a.out_pairsims) a.out_pairsims[o] = negm;
                }
            }
        if (a.want == ASPIRE_OT_PLAN_SIM) score = wave_sum(acc);
    }
    // a document longer than the launcher's tile bound would have been truncated silently: poison it
    if (q_len > 8 * T || c_len > 8 * T) score = __builtin_nanf("");
    if (lane == 0) a.scores[p] = score;
    if (a.out_qdistr) {
#pragma unroll
        for (int t = 0; t < T; ++t)
            if (lj == 0 && t * 8 + li < a.q.ext) a.out_qdistr[p * a.q.ext + t * 8 + li] = wa[t];
    }
    if (a.out_cdistr) {
#pragma unroll
        for (int t = 0; t < T; ++t)
            if (li == 0 && t * 8 + lj < a.c.ext) a.out_cdistr[p * a.c.ext + t * 8 + lj] = wb[t];
    }
}

// Kernel 2: one wave = one Sinkhorn solve, four pairs per workgroup; only registers and cross-lane ops.
// ~50 VGPRs at T = 1, so up to 8 solves share a SIMD and hide each other's cross-lane / transcendental
// latencies.
template <int T>
__global__ void __launch_bounds__(256) sinkhorn_kernel(ScoreArgs a, PairWs<T> ws, int64_t n_slots) {
    // this kernel is ONE long dependent chain per wave: when it shares a SIMD with throughput work of another launch
    // (a cost kernel of the next query), its instructions should issue first
    __builtin_amdgcn_s_setprio(3);
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    int64_t slot = (int64_t)blockIdx.x * 4 + wave;
    if (a.pairing == kPairMapped) {              // the slots of jobs [job0, job1); the grid is sized from an upper bound
        slot += a.job_off[a.job0];
        n_slots = a.job_off[a.job1];
    }
    if (slot < n_slots) {
        const PairIdx ix = pair_of_slot(a, slot);
        PairState<T> st;
        load_pair<T>(st, ws, slot, lane, a.cost_from_neg != 0);
        const float diam = a.diameter == nullptr ? fmaxf(sqrtf(ws.diam2[slot]), kMinDiameter) : group_diameter_of(a, ix);
        sinkhorn_pair<T>(a, st, a.q.len[ix.q_idx], a.c.len[ix.c_idx], diam, ix.p, lane);
    }
}

// ---------------------------------------------------------------------------------------------
// One wave = one PAIR, costs and solve in ONE launch (documents of <= 8 rows, CSR, a few dozen to a few thousand pairs: the
// per-query call of evaluate.py:58-76 -- one query against its pool of ~10^2 .. 10^3 candidates).  The two-launch form
// (pair_cost1_kernel: three waves per pair + sinkhorn_kernel<1>) costs a workspace round trip and a dependent launch: 12.1 + 7.5 us
// of kernels and ~3.5 us between them at 1 x 1000.  Here a wave
//   * issues ALL 24 loads of its candidate's rows at once (one HBM round trip; lane l owns coordinates 4 l + 256 s, s = 0 .. 2, of
//     every row), reads the query's rows (L2) stage by stage,
//   * accumulates the 64 dot products as 64 per-lane partial sums (each lane: all 8 x 8 pairs of rows over ITS twelve coordinates),
//     the 16 squared norms and the joint box's extent (all sixteen rows of a coordinate sit in one lane),
//   * folds them across the wave with the halving butterfly (common.h: butterfly_sum) so that lane l ends up with entry
//     lane_ij<1>(l) -- the layout sinkhorn_pair<1> solves in -- and goes straight on to the solve.
// Entries where the expansion cancels take -cdist and geomloss's cost from the exact sum, as everywhere (round 5).
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) pair_one_kernel(ScoreArgs a, int64_t n_slots) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    int64_t slot = (int64_t)blockIdx.x * 4 + wave;
    if (a.pairing == kPairMapped) {
        slot += a.job_off[a.job0];
        n_slots = a.job_off[a.job1];
    }
    if (slot < n_slots) {
    const PairIdx ix = pair_of_slot(a, slot);
    const int q_len = a.q.len[ix.q_idx], c_len = a.c.len[ix.c_idx];
    const float* qdoc = a.q.rows + (size_t)a.q.start[ix.q_idx] * kD;
    const float* cdoc = a.c.rows + (size_t)a.c.start[ix.c_idx] * kD;
    float4 y[3][8];
#pragma unroll
    for (int s = 0; s < 3; ++s)
#pragma unroll
        for (int r = 0; r < 8; ++r) y[s][r] = ld4_stream(cdoc + (size_t)min(r, c_len - 1) * kD + 4 * lane + 256 * s);   // pad rows: copies of the last
    float acc[64];
#pragma unroll
    for (int e = 0; e < 64; ++e) acc[e] = 0.f;
    float nrm[16];
#pragma unroll
    for (int e = 0; e < 16; ++e) nrm[e] = 0.f;
    float dsq = 0.f;
#pragma unroll
    for (int s = 0; s < 3; ++s) {
        float4 x[8];
#pragma unroll
        for (int r = 0; r < 8; ++r) x[r] = ld4(qdoc + (size_t)min(r, q_len - 1) * kD + 4 * lane + 256 * s);
        if (a.center) {
            // rows that share a large common component: the mean of the (padded) query rows comes off every row (fused.hip)
            float4 mu = x[0];
#pragma unroll
            for (int r = 1; r < 8; ++r) { mu.x += x[r].x; mu.y += x[r].y; mu.z += x[r].z; mu.w += x[r].w; }
            mu.x *= 0.125f; mu.y *= 0.125f; mu.z *= 0.125f; mu.w *= 0.125f;
#pragma unroll
            for (int r = 0; r < 8; ++r) {
                x[r].x -= mu.x; x[r].y -= mu.y; x[r].z -= mu.z; x[r].w -= mu.w;
                y[s][r].x -= mu.x; y[s][r].y -= mu.y; y[s][r].z -= mu.z; y[s][r].w -= mu.w;
            }
        }
        float4 mn = x[0], mx = x[0];
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            nrm[r] += sq4(x[r]);
            nrm[8 + r] += sq4(y[s][r]);
            const float4 u = x[r], v = y[s][r];
            mn.x = fminf(mn.x, fminf(u.x, v.x)); mn.y = fminf(mn.y, fminf(u.y, v.y)); mn.z = fminf(mn.z, fminf(u.z, v.z)); mn.w = fminf(mn.w, fminf(u.w, v.w));
            mx.x = fmaxf(mx.x, fmaxf(u.x, v.x)); mx.y = fmaxf(mx.y, fmaxf(u.y, v.y)); mx.z = fmaxf(mx.z, fmaxf(u.z, v.z)); mx.w = fmaxf(mx.w, fmaxf(u.w, v.w));
        }
        const float dx = mx.x - mn.x, dy = mx.y - mn.y, dz = mx.z - mn.z, dw = mx.w - mn.w;
        dsq = fmaf(dw, dw, fmaf(dz, dz, fmaf(dy, dy, fmaf(dx, dx, dsq))));
#pragma unroll
        for (int e = 0; e < 64; ++e) {
            // element e of the butterfly = the entry lane e will own: lane_ij<1>
            const int ej = (e & 3) | ((e >> 2) & 4), ei = ((e >> 2) & 3) | ((e >> 3) & 4);
            acc[e] = fmaf(x[ei].w, y[s][ej].w, fmaf(x[ei].z, y[s][ej].z, fmaf(x[ei].y, y[s][ej].y, fmaf(x[ei].x, y[s][ej].x, acc[e]))));
        }
    }
    const float dot = butterfly_sum<64>(acc, lane);
    const float nsum = butterfly_sum<16>(nrm, lane);              // lane l: element l >> 2 (0 .. 7 = |x_i|^2, 8 .. 15 = |y_j|^2)
    const float diam2 = wave_sum(dsq);
    int li, lj;
    lane_ij<1>(lane, li, lj);
    const float xx = __shfl(nsum, 4 * li), yy = __shfl(nsum, 32 + 4 * lj);
    const float sq = fmaf(-2.f, dot, xx) + yy, ns = xx + yy;
    PairState<1> st;
    st.cost[0][0] = cost_of_d2(sq);
    st.neg[0][0] = neg_of_expansion(sq);
    unsigned long long todo = __ballot(li < q_len && lj < c_len && expansion_cancels(sq, ns));       // (the rule and the exact sum: exact_d2.h)
    while (todo != 0) {        // rare: the whole wave on one entry (form A), from the rows as they are in memory (a common shift drops out)
        const int o = (int)__builtin_ctzll(todo);
        todo &= todo - 1;
        int oi, oj;
        lane_ij<1>(o, oi, oj);
        float4 u[3], v[3];
#pragma unroll
        for (int t = 0; t < 3; ++t) {
            u[t] = ld4(qdoc + (size_t)oi * kD + 4 * lane + 256 * t);
            v[t] = ld4(cdoc + (size_t)oj * kD + 4 * lane + 256 * t);
        }
        const float tot = wave_sum(wave_d2_part(u, v));
        if (lane == o) {
            st.neg[0][0] = -sqrtf(tot);
            st.cost[0][0] = cost_of_d2(tot);
        }
    }
    const float diam = a.diameter == nullptr ? fmaxf(sqrtf(diam2), kMinDiameter) : group_diameter_of(a, ix);
    sinkhorn_pair<1>(a, st, q_len, c_len, diam, ix.p, lane);
    }
}


// ---------------------------------------------------------------------------------------------
// Kernel 2, block form (throughput form for big grids, any T): a pair occupies LD x LD lanes of one DPP row and
// lane (li, lj) owns the R x R block of entries (R li + x, R lj + y), LD * R = 8 T:
//     T = 1: LD 2, R 4 (16 solves per wave) or LD 1, R 8 (64);  T = 2: LD 4, R 3 / 4 (4 solves per wave) or LD 2, R 6 / 8 (16);
//     T = 3, 4: LD 4, R 5 .. 8 (4 solves per wave)
// so most of a reduction is in-register adds and the cross-lane part is 1-2 DPP levels per direction.  The update
// is written around ONE exponential per entry, K_ij = exp2((f_i + g_j - C_ij) * log2(e)/eps):
//     sum_j b_j K_ij = exp((f_i - ft_i)/eps)   =>   ft_i = f_i - eps ln2 log2(sum_j b_j K_ij)
//     sum_i a_i K_ij = exp((g_j - gt_j)/eps)   =>   gt_j = g_j - eps ln2 log2(sum_i a_i K_ij)
// (the log-sum-exp of sinkhorn_pair::step2 shifted by the previous potential, with the marginal weights a, b as
// plain factors instead of log-weights inside the exponent), and the averaged update collapses to one FMA,
// f_i <- f_i - h log2(.), h = eps ln2 / 2 (eps ln2 for the final extrapolation, 0 once a pair has run out of
// steps while its wave mates have not).  Per step that is R^2 exp2 + 2R log2 per lane against 2 R^2 exp2 before.
// Every pair follows its own epsilon schedule; the per-step constants are two exp2 of an affine function of the
// step index (fp32: a relative 1e-7 on an intermediate temperature is far below the tolerance), no table.
// A sum that leaves fp32 range (extreme scaling) poisons the score with NaN; sinkhorn_repair_kernel then redoes
// such pairs with the max-shifted solver.
// ---------------------------------------------------------------------------------------------
typedef float f2v __attribute__((ext_vector_type(2)));     // a register pair for the packed fp32 instructions

template <int LD>
__device__ __forceinline__ float blk_sum_j(float v) {   // all-reduce over the LD lanes that share li
    if constexpr (LD >= 2) v += lane_xor<1>(v);
    if constexpr (LD == 4) v += lane_xor<2>(v);
    return v;
}
template <int LD>
__device__ __forceinline__ float blk_max_j(float v) {
    if constexpr (LD >= 2) v = fmaxf(v, lane_xor<1>(v));
    if constexpr (LD == 4) v = fmaxf(v, lane_xor<2>(v));
    return v;
}
template <int LD>
__device__ __forceinline__ float blk_sum_i(float v) {   // all-reduce over the LD lanes that share lj
    if constexpr (LD == 1) {
        return v;
    } else if constexpr (LD == 2) {
        return v + lane_xor<2>(v);
    } else {
        v += dpp_mov<0x124>(v, v);       // row_ror:4
        return v + dpp_mov<0x128>(v, v); // row_ror:8
    }
}
template <int LD>
__device__ __forceinline__ float blk_max_i(float v) {
    if constexpr (LD == 1) {
        return v;
    } else if constexpr (LD == 2) {
        return fmaxf(v, lane_xor<2>(v));
    } else {
        v = fmaxf(v, dpp_mov<0x124>(v, v));
        return fmaxf(v, dpp_mov<0x128>(v, v));
    }
}

template <int T, int LD, int R>
__global__ void __launch_bounds__(256) sinkhorn_block_kernel(ScoreArgs a, PairWs<T> ws, int64_t n_slots) {
    static_assert(LD * R <= 8 * T && LD * R > 8 * (T - 1), "block layout must fit the 8T x 8T slot");
    constexpr int NL = LD * LD, PPW = 64 / NL, E = 64 * T * T, LDS_ = 8 * T;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int pp = lane / NL, lp = lane % NL, li = lp / LD, lj = lp % LD;
    int64_t slot0 = ((int64_t)blockIdx.x * 4 + wave) * PPW;
    if (a.pairing == kPairMapped) {              // the slots of jobs [job0, job1); the grid is sized from an upper bound
        slot0 += a.job_off[a.job0];
        n_slots = a.job_off[a.job1];
    }
    if (slot0 >= n_slots) return;
    bool real = slot0 + pp < n_slots;                        // tail wave: surplus groups redo the last pair, store nothing
    int64_t slot = real ? slot0 + pp : n_slots - 1;
    PairIdx ix = pair_of_slot(a, slot);
    int q_len = a.q.len[ix.q_idx], c_len = a.c.len[ix.c_idx];
    if (gate_few_long(a)) {
        // hybrid (score_types.h): only the pairs the fused kernel left to the 16-row kernels have slots.  The other lane
        // groups of the wave mirror its first such pair (their own slots hold nothing: a garbage diameter could mean any
        // number of steps) and store nothing.
        real = real && (q_len > 8 || c_len > 8);
        const unsigned long long todo = __ballot(real);
        if (todo == 0) return;
        const int lead = (int)__builtin_ctzll(todo);
        const int lo = __builtin_amdgcn_readlane((int)(uint32_t)slot, lead), hi = __builtin_amdgcn_readlane((int)(slot >> 32), lead);
        if (!real) slot = ((int64_t)hi << 32) | (uint32_t)lo;
        ix = pair_of_slot(a, slot);
        q_len = a.q.len[ix.q_idx];
        c_len = a.c.len[ix.c_idx];
    }
    const int64_t p = ix.p;

    float cost[R][R];
    bool rv[R], cv[R];
#pragma unroll
    for (int t = 0; t < R; ++t) {
        rv[t] = R * li + t < q_len;
        cv[t] = R * lj + t < c_len;
    }
    // Entries outside the pair's q_len x c_len rectangle are never written by some producers (and are masked by
    // zero weights here): read them as 0 so that no stale inf / nan can reach a sum through 0 * x.
    auto load_block = [&](const float* base, float (&dst)[R][R]) {
#pragma unroll
        for (int x = 0; x < R; ++x) {
            const float* row = base + slot * E + (R * li + x) * LDS_ + R * lj;
            if constexpr (R % 4 == 0) {
#pragma unroll
                for (int y = 0; y < R; y += 4) {
                    const float4 v = ld4(row + y);
                    dst[x][y] = v.x; dst[x][y + 1] = v.y; dst[x][y + 2] = v.z; dst[x][y + 3] = v.w;
                }
            } else if constexpr (R % 2 == 0) {
#pragma unroll
                for (int y = 0; y < R; y += 2) {
                    const float2 v = *reinterpret_cast<const float2*>(row + y);
                    dst[x][y] = v.x; dst[x][y + 1] = v.y;
                }
            } else {
#pragma unroll
                for (int y = 0; y < R; ++y) dst[x][y] = row[y];
            }
#pragma unroll
            for (int y = 0; y < R; ++y) dst[x][y] = (rv[x] && cv[y]) ? dst[x][y] : 0.f;
        }
    };
    // ---- marginals (pair_distances.py:57-60) from -cdist; only the weights survive this scope -----------------
    const float temp = (float)a.temp;
    float wa[R], wb[R];
    {
        load_block(ws.neg, cost);   // borrowed: holds -cdist here
        float qm[R], cm[R];
#pragma unroll
        for (int x = 0; x < R; ++x) {
            float m = kNegBig;
#pragma unroll
            for (int y = 0; y < R; ++y) m = fmaxf(m, (rv[x] && cv[y]) ? cost[x][y] : kNegBig);
            qm[x] = blk_max_j<LD>(m) / temp;
        }
#pragma unroll
        for (int y = 0; y < R; ++y) {
            float m = kNegBig;
#pragma unroll
            for (int x = 0; x < R; ++x) m = fmaxf(m, (rv[x] && cv[y]) ? cost[x][y] : kNegBig);
            cm[y] = blk_max_i<LD>(m) / temp;
        }
        float mq = kNegBig, mc = kNegBig;
#pragma unroll
        for (int t = 0; t < R; ++t) {
            mq = fmaxf(mq, rv[t] ? qm[t] : kNegBig);
            mc = fmaxf(mc, cv[t] ? cm[t] : kNegBig);
        }
        mq = blk_max_i<LD>(mq);
        mc = blk_max_j<LD>(mc);
        float sq = 0.f, sc = 0.f;
#pragma unroll
        for (int t = 0; t < R; ++t) {
            sq += rv[t] ? fast_exp(qm[t] - mq) : 0.f;
            sc += cv[t] ? fast_exp(cm[t] - mc) : 0.f;
        }
        const float lsq = fast_log(blk_sum_i<LD>(sq)), lsc = fast_log(blk_sum_j<LD>(sc));
#pragma unroll
        for (int t = 0; t < R; ++t) {
            wa[t] = rv[t] ? fast_exp(qm[t] - mq - lsq) : 0.f;   // log_softmax(...).exp(); zero weight == geomloss's
            wb[t] = cv[t] ? fast_exp(cm[t] - mc - lsc) : 0.f;   // log-weight -100000
        }
    }
    if (a.cost_from_neg) {      // `cost` still holds the pair's -cdist block (zeros outside its rectangle)
#pragma unroll
        for (int x = 0; x < R; ++x)
#pragma unroll
            for (int y = 0; y < R; ++y) cost[x][y] = (rv[x] && cv[y]) ? cost_of_dist(-cost[x][y]) : 0.f;
    } else {
        load_block(ws.cost, cost);
    }
    const float diam = a.diameter == nullptr ? fmaxf(sqrtf(ws.diam2[slot]), kMinDiameter) : group_diameter_of(a, ix);
    // ---- epsilon schedule: step 0 = diam, 1 .. n_mid = exp(ld + (k-1) lsc), n_mid+1 = blur, n_mid+2 = blur (final)
    float ldf;
    const int n_mid = schedule_mid_steps(a, diam, ldf);
    const int n_steps = n_mid + 3;
    int max_steps = n_steps;
#pragma unroll
    for (int m = NL; m < 64; m <<= 1) max_steps = max(max_steps, __shfl_xor(max_steps, m));
    const float r2_first = kLog2e * rcp_refined(diam), h_first = 0.5f * kLn2 * diam;
    const float eb = (float)a.blur;
    const float r2_blur = kLog2e * rcp_refined(eb), h_blur = 0.5f * kLn2 * eb;

    // ---- initialisation at eps = diam: softmin of the bare weights.  No shift is needed: the largest weight of a
    // probability vector over <= 32 atoms is >= 1/32 and C/diam <= ~1, so the sums stay in range. --------------
    float f[R], g[R];
    {
        float rs[R], cs[R];
#pragma unroll
        for (int t = 0; t < R; ++t) rs[t] = cs[t] = 0.f;
#pragma unroll
        for (int x = 0; x < R; ++x)
#pragma unroll
            for (int y = 0; y < R; ++y) {
                const float k0 = __builtin_amdgcn_exp2f(-cost[x][y] * r2_first);
                rs[x] = fmaf(wb[y], k0, rs[x]);
                cs[y] = fmaf(wa[x], k0, cs[y]);
            }
#pragma unroll
        for (int t = 0; t < R; ++t) {
            f[t] = -2.f * h_first * __builtin_amdgcn_logf(blk_sum_j<LD>(rs[t]));
            g[t] = -2.f * h_first * __builtin_amdgcn_logf(blk_sum_i<LD>(cs[t]));
        }
    }
    // ---- the annealing loop ---------------------------------------------------------------------------------
    // One step on register PAIRS (v_pk_mul / v_pk_fma_f32 work on two entries at once): the entries of a row as R / 2 column
    // pairs (+ a single for odd R).  R = 4: 76 issue slots per step instead of 122, R = 3: 62 instead of 90 -- the kernel
    // runs at its VALU-issue roof (profiles/sinkhorn_roofline.json), so only fewer instructions make it faster.  The
    // per-step constants follow from the previous step's by one multiply each through the annealed part of the schedule
    // (steps 2 .. n_mid: eps *= scaling), with a select-free loop while all of the wave's pairs anneal.
    constexpr int RP = R / 2;
    constexpr bool ODD = (R & 1) != 0;
    f2v cp[R][RP > 0 ? RP : 1], wbp[RP > 0 ? RP : 1], gp[RP > 0 ? RP : 1];
#pragma unroll
    for (int j = 0; j < RP; ++j) {
        wbp[j] = f2v{wb[2 * j], wb[2 * j + 1]};
        gp[j] = f2v{g[2 * j], g[2 * j + 1]};
#pragma unroll
        for (int x = 0; x < R; ++x) cp[x][j] = f2v{cost[x][2 * j], cost[x][2 * j + 1]};
    }
    float go = ODD ? g[R - 1] : 0.f;
    auto step = [&](float r2, float h) {
        f2v g2p[RP > 0 ? RP : 1], csp[RP > 0 ? RP : 1];
        float rs[R], cso = 0.f;
        const float g2o = go * r2;
#pragma unroll
        for (int j = 0; j < RP; ++j) {
            g2p[j] = gp[j] * r2;
            csp[j] = f2v{0.f, 0.f};
        }
#pragma unroll
        for (int x = 0; x < R; ++x) {
            const float fx = f[x] * r2;
            f2v racc = {0.f, 0.f};
#pragma unroll
            for (int j = 0; j < RP; ++j) {
                const f2v arg = __builtin_elementwise_fma(cp[x][j], f2v{-r2, -r2}, f2v{fx, fx} + g2p[j]);
                const f2v kk = {__builtin_amdgcn_exp2f(arg.x), __builtin_amdgcn_exp2f(arg.y)};
                racc = __builtin_elementwise_fma(kk, wbp[j], racc);
                csp[j] = __builtin_elementwise_fma(kk, f2v{wa[x], wa[x]}, csp[j]);
            }
            rs[x] = racc.x + racc.y;
            if constexpr (ODD) {
                const float ko = __builtin_amdgcn_exp2f(fmaf(-cost[x][R - 1], r2, fx + g2o));
                rs[x] = fmaf(wb[R - 1], ko, rs[x]);
                cso = fmaf(wa[x], ko, cso);
            }
        }
#pragma unroll
        for (int x = 0; x < R; ++x) f[x] = fmaf(-h, __builtin_amdgcn_logf(blk_sum_j<LD>(rs[x])), f[x]);
#pragma unroll
        for (int j = 0; j < RP; ++j) {
            const f2v lc = {__builtin_amdgcn_logf(blk_sum_i<LD>(csp[j].x)), __builtin_amdgcn_logf(blk_sum_i<LD>(csp[j].y))};
            gp[j] = __builtin_elementwise_fma(f2v{-h, -h}, lc, gp[j]);
        }
        if constexpr (ODD) go = fmaf(-h, __builtin_amdgcn_logf(blk_sum_i<LD>(cso)), go);
    };
    {
        const float scal = (float)a.scaling, inv_scal = (float)(1.0 / a.scaling);
        int n_mid_lo = n_mid;
#pragma unroll
        for (int m = NL; m < 64; m <<= 1) n_mid_lo = min(n_mid_lo, __shfl_xor(n_mid_lo, m));
        n_mid_lo = __builtin_amdgcn_readfirstlane(n_mid_lo);
        max_steps = __builtin_amdgcn_readfirstlane(max_steps);
        float r2 = r2_first, h = h_first;
        int k = 0;
        // eps_k: diam at k = 0 and 1, diam scaling^(k-1) up to k = n_mid, then blur (averaged), blur (final, h doubled), and
        // nothing (h = 0) while a wave mate with a longer schedule is still annealing
        auto general = [&](int upto) {
#pragma unroll 1
            for (; k < upto; ++k) {
                const bool anneal = k >= 2 && k <= n_mid;
                r2 = anneal ? r2 * inv_scal : r2;
                h = anneal ? h * scal : h;
                if (k > n_mid) { r2 = r2_blur; h = k == n_mid + 1 ? h_blur : (k == n_mid + 2 ? 2.f * h_blur : 0.f); }
                step(r2, h);
            }
        };
        general(min(max_steps, 2));
        const int fast_end = min(max_steps, n_mid_lo + 1);
#pragma unroll 1
        for (; k < fast_end; ++k) {
            r2 *= inv_scal;
            h *= scal;
            step(r2, h);
        }
        general(max_steps);
    }
#pragma unroll
    for (int j = 0; j < RP; ++j) {
        g[2 * j] = gp[j].x;
        g[2 * j + 1] = gp[j].y;
    }
    if constexpr (ODD) g[R - 1] = go;
    // ---- outputs ---------------------------------------------------------------------------------------------
    float score;
    if (a.want != ASPIRE_OT_PLAN_SIM) {
        float acc = 0.f;
#pragma unroll
        for (int t = 0; t < R; ++t) {
            acc += (lj == 0 && rv[t]) ? wa[t] * f[t] : 0.f;
            acc += (li == 0 && cv[t]) ? wb[t] * g[t] : 0.f;
        }
        score = blk_sum_i<LD>(blk_sum_j<LD>(acc));
        if (a.want == ASPIRE_OT_SIMILARITY) score = -score;
    } else {
        const float rb = rcp_refined(eb);
        load_block(ws.neg, cost);
        float acc = 0.f;
#pragma unroll
        for (int x = 0; x < R; ++x)
#pragma unroll
            for (int y = 0; y < R; ++y) {
                const bool valid = rv[x] && cv[y];
                const float negm = valid ? cost[x][y] : 0.f;
                const float outer = valid ? f[x] + g[y] : 0.f;
                acc += fast_exp(div_r(outer + negm, eb, rb)) * (wa[x] * wb[y]) * negm;
            }
        score = blk_sum_i<LD>(blk_sum_j<LD>(acc));
    }
    // an overflowed / vanished sum sticks to the potentials as inf / nan: poison the pair (sinkhorn_repair_kernel re-solves it)
    if (!(fabsf(score) < 1e30f) || q_len > LD * R || c_len > LD * R) score = __builtin_nanf("");
    if (real && lp == 0) a.scores[p] = score;
}

// Pairs the block form poisoned (NaN score) are solved again, one wave each, by the max-shifted solver.
template <int T>
__global__ void __launch_bounds__(256) sinkhorn_repair_kernel(ScoreArgs a, PairWs<T> ws, int64_t n_slots) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    int64_t base = ((int64_t)blockIdx.x * 4 + wave) * 64;
    if (a.pairing == kPairMapped) {
        base += a.job_off[a.job0];
        n_slots = a.job_off[a.job1];
    }
    if (base >= n_slots) return;
    bool bad = false;
    if (base + lane < n_slots) {
        const PairIdx ix = pair_of_slot(a, base + lane);
        const float s = a.scores[ix.p];
        bad = !(fabsf(s) < 1e30f);
        // hybrid, few long pairs: only those have slots in the workspace (the fused kernel re-solves its own overflowed pairs)
        if (gate_few_long(a) && a.q.len[ix.q_idx] <= 8 && a.c.len[ix.c_idx] <= 8) bad = false;
    }
    unsigned long long todo = __ballot(bad);
    while (todo) {
        const int k = __builtin_ctzll(todo);
        todo &= todo - 1;
        const int64_t slot = base + k;
        const PairIdx ix = pair_of_slot(a, slot);
        PairState<T> st;
        load_pair<T>(st, ws, slot, lane, a.cost_from_neg != 0);
        const float diam = a.diameter == nullptr ? fmaxf(sqrtf(ws.diam2[slot]), kMinDiameter) : group_diameter_of(a, ix);
        sinkhorn_pair<T>(a, st, a.q.len[ix.q_idx], a.c.len[ix.c_idx], diam, ix.p, lane);
    }
}

}  // namespace

// ---------------------------------------------------------------------------------------------
// host side: the launchers (score_types.h)
// ---------------------------------------------------------------------------------------------
// ---- stage 2: one Sinkhorn solve per workspace slot.  n_slots: the slots of this launch (MAPPED: an upper bound, the
// kernels read the exact range of jobs [a.job0, a.job1) from job_off). --------------------------------------------------
// Which solver and how many lanes per pair: forms.hip (solver_form).
int launch_sinkhorn_stage(const ScoreArgs& a, int T_rt, float* cost, float* neg, float* diam2, int64_t n_slots, int max_rows, bool extra,
                          int form_hint, hipStream_t stream) {
    const SolveChoice ch = solver_form(T_rt, n_slots, max_rows, extra, form_hint);
    return dispatch_T(8 * T_rt, [&](auto tc) -> int {
        constexpr int T = decltype(tc)::value;
        const PairWs<T> ws{cost, neg, diam2};
        if (ch.kernel == Solver::Block) {
            // the layouts that are built: LD lanes per pair side, R entries per lane side, LD * R rows within this T's last tile
            auto launch_block = [&](auto ldc, auto rc) {
                constexpr int LD = decltype(ldc)::value, R = decltype(rc)::value, PPB = 4 * 64 / (LD * LD);
                if constexpr (LD * R <= 8 * T && LD * R > 8 * (T - 1)) {
                    if (ch.lanes == LD && ch.per_lane == R)
                        hipLaunchKernelGGL((sinkhorn_block_kernel<T, LD, R>), dim3((unsigned)((n_slots + PPB - 1) / PPB)),
                                           dim3(256), 0, stream, a, ws, n_slots);
                }
            };
            using I2 = std::integral_constant<int, 2>;
            using I4 = std::integral_constant<int, 4>;
            launch_block(std::integral_constant<int, 1>{}, std::integral_constant<int, 8>{});
            launch_block(I2{}, I4{});
            launch_block(I2{}, std::integral_constant<int, 6>{});
            launch_block(I2{}, std::integral_constant<int, 8>{});
            launch_block(I4{}, I2{});
            launch_block(I4{}, std::integral_constant<int, 3>{});
            launch_block(I4{}, I4{});
            launch_block(I4{}, std::integral_constant<int, 5>{});
            launch_block(I4{}, std::integral_constant<int, 6>{});
            launch_block(I4{}, std::integral_constant<int, 7>{});
            launch_block(I4{}, std::integral_constant<int, 8>{});
            ASPIRE_LAUNCH_OK();
            if (ch.repair)
                hipLaunchKernelGGL(sinkhorn_repair_kernel<T>, dim3((unsigned)((n_slots + 255) / 256)), dim3(256), 0, stream, a, ws,
                                   n_slots);
        } else {
            hipLaunchKernelGGL(sinkhorn_kernel<T>, dim3((unsigned)((n_slots + 3) / 4)), dim3(256), 0, stream, a, ws, n_slots);
        }
        ASPIRE_LAUNCH_OK();
        return (int)ASPIRE_OK;
    });
}

// costs and solve of `n_slots` pairs of documents of <= 8 rows in one launch, one wave per pair (MAPPED: the pairs of jobs
// [a.job0, a.job1), n_slots an upper bound)
int launch_pair_one(const ScoreArgs& a, int64_t n_slots, hipStream_t stream) {
    hipLaunchKernelGGL(pair_one_kernel, dim3((unsigned)((n_slots + 3) / 4)), dim3(256), 0, stream, a, n_slots);
    ASPIRE_LAUNCH_OK();
    return ASPIRE_OK;
}

}  // namespace aspire
