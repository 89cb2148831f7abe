// Backward of the otAspire distance (include/aspire_hip.h, aspire_ot_backward_f32): the gradient of a pair's OT_eps value with respect
// to its query and candidate sentence rows -- what the reference's autograd gives for the train-time branch of
// AllPairMaskedWasserstein.compute_distance (pair_distances.py:88-92) under its triplet loss.
//
// A RESTATEMENT: geomloss 0.2.4 is not vendored and its Sinkhorn solver is "parity unpinned" here (NOTES.md), so this is
// the gradient of what geomloss's sinkhorn_tensorized does for SamplesLoss("sinkhorn", p=1, debias=False, potentials=False), read
// from its published source: the costs are C_xy = cost(x, y.detach()) and C_yx = cost(y, x.detach()); the whole eps-scaling loop
// runs with grad disabled; only the last extrapolation runs with grad, on (a_log + b_x / eps).detach() and
// (b_log + a_y / eps).detach(); the value is <a, b_x> + <b, a_y> with a, b (the reference's soft-max marginals) NOT detached;
// max_diameter is an .item(), a constant.  Per pair, with gs = dLoss / dscore, a / b the marginals, la / lb geomloss's log-weights,
// eps = blur, f0 / g0 the potentials after the last averaged step, tau = sent_sm_temp:
//   f_i = -eps LSE_j(lb_j + (g0_j - C_ij) / eps)      g_j = -eps LSE_i(la_i + (f0_i - C_ij) / eps)        (the last extrapolation)
//   C_ij = sqrt(max(d_ij^2, 1e-8))                     s_ij = -d_ij   (the torch.cdist block the marginals are built from)
//   W_ij = exp(lb_j + (g0_j - C_ij + f_i) / eps)       (every row i sums to 1)
//   V_ij = exp(la_i + (f0_i - C_ij + g_j) / eps)       (every column j sums to 1)
//   u_i  = a_i (f_i - sum_k a_k f_k) / tau   at entry (i, j*(i)),  j*(i) = the FIRST arg-max over j of s_ij in the valid block
//   v_j  = b_j (g_j - sum_l b_l g_l) / tau   at entry (i*(j), j),  i*(j) = the first arg-max over i
//   M_ij = u_i [j == j*(i)] + v_j [i == i*(j)]
//   grad_x_i = gs sum_j ( a_i W_ij [d_ij^2 > 1e-8] / C_ij  -  M_ij [d_ij > 0] / d_ij ) (x_i - y_j)
//   grad_y_j = gs sum_i ( M_ij [d_ij > 0] / d_ij  -  b_j V_ij [d_ij^2 > 1e-8] / C_ij ) (x_i - y_j)
// x receives the transport term through f only and y through g only (the detach pattern); both receive the marginal term.  For
// ASPIRE_OT_SIMILARITY the sign flips.
//
// The frame -- one workgroup of four waves per pair, a lane's 12 coordinates, poisoned, empty and pad rows -- is pair_bwd.h's.
//   1  distances: d_ij from the DIRECT differences into one LDS block over the valid entries (row stride cl | 1: odd, so that a
//      thread per row and a thread per column both read it without bank conflicts).  C = max(d, 1e-4) and s = -d both come from it --
//      direct differences everywhere, not the matmul expansion of generic.hip: the gradient is taken where training drives rows
//      together, and the expansion cancels there.
//   2  the solve: generic.hip's, restated (geomloss's own formulation) -- marginals, log-weights with the -100000 rule, kMinDiameter,
//      the float64 schedule exp(ldm + k log_scaling), max-shifted log-sum-exps with expf / logf -- with threads 0 .. 127 on the rows
//      and 128 .. 255 on the columns; f0 / g0 are kept in front of the last extrapolation, j*(i) / i*(j) are recorded while the row
//      and column maxima of the marginals are formed.  The diameter is diameter[p / diam_group], or the box of the pair's own
//      valid rows when diameter == NULL, exactly as the forward reads it.  One departure, for fp32's sake: the solve runs on
//      C - c0, c0 = the smallest cost of the pair's block.  That is an exact reparametrisation (every potential comes out c0 / 2
//      lower, and W, V, u, v only read f + g - C and differences of f or of g), but the potentials of random 768-d rows are then of
//      size 1 instead of 10, and their rounding, which the exponent multiplies by 1 / eps, shrinks with them: the fp32 emulation of
//      these formulas on the test's 8 x 8 pairs is 1.3e-7 from float64 with the shift and 6.5e-7 without.
//   3  rows: W_ij / V_ij are wave-uniform scalars recomputed from the vectors in LDS while a row's partners stream past (one expf
//      per entry beside a 3 KB row load), M stays two index vectors and two value vectors; w (x_i - y_j) is formed directly (NOT
//      rowsum x_i - sum_j w y_j: that cancels between near-equal rows); every row is written once with 16-byte stores.
#include "pair_bwd.h"

namespace aspire {
namespace {

constexpr int kOtBwdSide = kPairBwdThreads / 2;      // rows | columns

// the 256 threads' sum in one fixed order (every thread calls; `red` = 256 floats): generic.hip's block_reduce
__device__ __forceinline__ float block_sum(float v, float* red) {
    const int tid = threadIdx.x;
    red[tid] = v;
    __syncthreads();
    for (int s = kPairBwdThreads / 2; s > 0; s >>= 1) {
        if (tid < s) red[tid] = red[tid] + red[tid + s];
        __syncthreads();
    }
    const float r = red[0];
    __syncthreads();
    return r;
}

__device__ __forceinline__ float block_min(float v, float* red) {
    const int tid = threadIdx.x;
    red[tid] = v;
    __syncthreads();
    for (int s = kPairBwdThreads / 2; s > 0; s >>= 1) {
        if (tid < s) red[tid] = fminf(red[tid], red[tid + s]);
        __syncthreads();
    }
    const float r = red[0];
    __syncthreads();
    return r;
}

struct OtBwdLds {         // offsets in floats into the dynamic LDS block
    int red, f, g, ft, gt, la, lb, wa, wb, u, v, jstar, istar, dist, total;
};
__host__ __device__ inline int ot_bwd_stride(int cols) { return cols | 1; }
__host__ __device__ inline OtBwdLds ot_bwd_layout(int rows_q, int rows_c) {
    OtBwdLds L;
    const int m = ((rows_q > rows_c ? rows_q : rows_c) + 3) & ~3;
    int o = 0;
    L.red = o; o += kPairBwdThreads;
    L.f = o; o += m;
    L.g = o; o += m;
    L.ft = o; o += m;
    L.gt = o; o += m;
    L.la = o; o += m;
    L.lb = o; o += m;
    L.wa = o; o += m;
    L.wb = o; o += m;
    L.u = o; o += m;
    L.v = o; o += m;
    L.jstar = o; o += m;
    L.istar = o; o += m;
    L.dist = o; o += rows_q * ot_bwd_stride(rows_c);
    L.total = o;
    return L;
}

struct OtBwdArgs {
    RepSet q, c;
    float blur, temp;
    double log_blur, log_scaling;        // natural logs, float64, formed on the host (schedule lengths)
    const float* diameter;
    int64_t diam_group;
    int want;
    const float* grad_scores;
    float* grad_q;
    float* grad_c;
};

__global__ void __launch_bounds__(kPairBwdThreads) ot_bwd_kernel(OtBwdArgs a, int rows_q, int rows_c) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t p = blockIdx.x;
    const PairFrame fr = pair_frame(a.q, a.c, a.grad_q, a.grad_c, p, rows_q, rows_c);
    if (skip_pair(fr, lane, wave)) return;
    const int ql = fr.ql, cl = fr.cl;
    const float *qdoc = fr.qdoc, *cdoc = fr.cdoc;
    float *gq = fr.gq, *gc = fr.gc;
    const OtBwdLds L = ot_bwd_layout(rows_q, rows_c);
    const int ld = ot_bwd_stride(cl);          // (the pair's own stride: ql * ld <= rows_q * (rows_c | 1))
    float* red = lds + L.red;
    float* dist = lds + L.dist;
    float* f = lds + L.f;                      // f0 / g0 once the loop is over
    float* g = lds + L.g;
    float* ft = lds + L.ft;                    // the last extrapolation's f / g in the end
    float* gt = lds + L.gt;
    float* la = lds + L.la;
    float* lb = lds + L.lb;
    float* wa = lds + L.wa;
    float* wb = lds + L.wb;
    float* u = lds + L.u;
    float* v = lds + L.v;
    int* jstar = reinterpret_cast<int*>(lds + L.jstar);
    int* istar = reinterpret_cast<int*>(lds + L.istar);
    const float gs = a.want == ASPIRE_OT_SIMILARITY ? -a.grad_scores[p] : a.grad_scores[p];

    // ---- 1  distances from direct differences ---------------------------------------------------------------------------------
    direct_distances(fr, dist, ld, lane, wave);
    // ---- diameter: the caller's (one per group) or the bounding box of the pair's own valid rows ------------------------------
    float diam;
    if (a.diameter != nullptr) {
        diam = a.diameter[p / a.diam_group];
        __syncthreads();
    } else {
        float acc = 0.f;
        for (int d = tid; d < kD; d += kPairBwdThreads) {
            float mn = INFINITY, mx = -INFINITY;
            for (int r = 0; r < ql; ++r) { const float w = qdoc[(size_t)r * kD + d]; mn = fminf(mn, w); mx = fmaxf(mx, w); }
            for (int r = 0; r < cl; ++r) { const float w = cdoc[(size_t)r * kD + d]; mn = fminf(mn, w); mx = fmaxf(mx, w); }
            acc += (mx - mn) * (mx - mn);
        }
        diam = sqrtf(block_sum(acc, red));      // (its first barrier also publishes the distance block)
    }
    diam = fmaxf(diam, kMinDiameter);
    // c0: the smallest cost of the block (the solve runs on C - c0, see the header)
    float c0 = INFINITY;
    for (int e = tid; e < ql * cl; e += kPairBwdThreads) c0 = fminf(c0, fmaxf(dist[(e / cl) * ld + e % cl], 1e-4f));
    c0 = block_min(c0, red);

    // ---- 2  the solve -----------------------------------------------------------------------------------------------------------
    // C = max(d, 1e-4) = sqrt(max(d^2, 1e-8)) (less c0),  s = -d.  Threads 0 .. 127 own a row each, 128 .. 255 a column each.
    const bool row_side = tid < kOtBwdSide;
    const int t = tid & (kOtBwdSide - 1);
    const float temp = a.temp;
    // marginals (pair_distances.py:57-60): soft-max over sentences of the best match / temp; the first arg-max is kept
    if (row_side) {
        if (t < ql) {
            float m = -INFINITY;
            int best = 0;
            for (int j = 0; j < cl; ++j) {
                const float s = -dist[t * ld + j];
                if (s > m) { m = s; best = j; }
            }
            ft[t] = m / temp;
            jstar[t] = best;
        }
    } else if (t < cl) {
        float m = -INFINITY;
        int best = 0;
        for (int i = 0; i < ql; ++i) {
            const float s = -dist[i * ld + t];
            if (s > m) { m = s; best = i; }
        }
        gt[t] = m / temp;
        istar[t] = best;
    }
    __syncthreads();
    {
        float mx = -INFINITY, sm = 0.f;
        const float* h = row_side ? ft : gt;
        const int n = row_side ? ql : cl;
        for (int k = 0; k < n; ++k) mx = fmaxf(mx, h[k]);
        for (int k = 0; k < n; ++k) sm += expf(h[k] - mx);
        const float ls = logf(sm);
        const float w = t < n ? expf(h[t] - mx - ls) : 0.f;          // log_softmax(...).exp()
        __syncthreads();
        if (t < n) {
            (row_side ? wa : wb)[t] = w;
            (row_side ? la : lb)[t] = w > 0.f ? logf(w) : -100000.f;   // geomloss log_weights
        }
    }
    __syncthreads();
    // Sinkhorn loop (geomloss sinkhorn_loop): softmin(eps, C, h)_i = -eps * LSE_j(h_j - C_ij / eps)
    // first: true = the initialisation (bare log-weights); else h = log-weight + potential / eps
    auto softmins = [&](float eps, bool first) {
        if (row_side) {
            if (t < ql) {           // ft_i = softmin over j
                float m = -INFINITY;
                for (int j = 0; j < cl; ++j) m = fmaxf(m, lb[j] + (first ? 0.f : g[j] / eps) - (fmaxf(dist[t * ld + j], 1e-4f) - c0) / eps);
                float s = 0.f;
                for (int j = 0; j < cl; ++j) s += expf(lb[j] + (first ? 0.f : g[j] / eps) - (fmaxf(dist[t * ld + j], 1e-4f) - c0) / eps - m);
                ft[t] = -eps * (m + logf(s));
            }
        } else if (t < cl) {        // gt_j = softmin over i
            float m = -INFINITY;
            for (int i = 0; i < ql; ++i) m = fmaxf(m, la[i] + (first ? 0.f : f[i] / eps) - (fmaxf(dist[i * ld + t], 1e-4f) - c0) / eps);
            float s = 0.f;
            for (int i = 0; i < ql; ++i) s += expf(la[i] + (first ? 0.f : f[i] / eps) - (fmaxf(dist[i * ld + t], 1e-4f) - c0) / eps - m);
            gt[t] = -eps * (m + logf(s));
        }
        __syncthreads();
    };
    auto update = [&](bool averaged) {
        if (row_side) {
            if (t < ql) f[t] = averaged ? 0.5f * (f[t] + ft[t]) : ft[t];
        } else if (t < cl) {
            g[t] = averaged ? 0.5f * (g[t] + gt[t]) : gt[t];
        }
        __syncthreads();
    };
    const float eb = a.blur;
    softmins(diam, true);
    update(false);
    softmins(diam, false);          // eps_s[0] = diam
    update(true);
    const double ldm = log((double)diam);
    int n_mid = (int)ceil((a.log_blur - ldm) / a.log_scaling);      // len(arange(log diam, log blur, log scaling))
    n_mid = n_mid < 0 ? 0 : n_mid;
    for (int k = 0; k < n_mid; ++k) {
        softmins((float)exp(ldm + (double)k * a.log_scaling), false);
        update(true);
    }
    softmins(eb, false);
    update(true);                   // f, g = f0, g0
    softmins(eb, false);            // last extrapolation: simultaneous, not averaged -- ft, gt = the forward's f, g; f0, g0 stay

    // u, v: the value's gradient with respect to the marginals' logits
    const float saf = block_sum(row_side && t < ql ? wa[t] * ft[t] : 0.f, red);
    const float sbg = block_sum(!row_side && t < cl ? wb[t] * gt[t] : 0.f, red);
    if (row_side) {
        if (t < ql) u[t] = wa[t] * (ft[t] - saf) / temp;
    } else if (t < cl) {
        v[t] = wb[t] * (gt[t] - sbg) / temp;
    }
    __syncthreads();

    // ---- 3  gradient rows -----------------------------------------------------------------------------------------------------
    const Row zero = splat(0.f);
    for (int i = wave; i < ql; i += kPairBwdWaves) {
        const Row x = load_row(qdoc + (size_t)i * kD, lane);
        const float a_i = wa[i], f_i = ft[i], u_i = u[i];
        const int js = jstar[i];
        Row acc = zero;
#pragma unroll 2
        for (int j = 0; j < cl; ++j) {
            const float d = dist[i * ld + j], C = fmaxf(d, 1e-4f);
            const float W = expf(lb[j] + (g[j] - (C - c0) + f_i) / eb);
            const float M = (j == js ? u_i : 0.f) + (istar[j] == i ? v[j] : 0.f);
            const float w = (d > 1e-4f ? a_i * W / C : 0.f) - (d > 0.f ? M / d : 0.f);
            add_diff(acc, w, x, load_row(cdoc + (size_t)j * kD, lane));
        }
        store_row(gq + (size_t)i * kD, lane, scaled(gs, acc));
    }
    for (int j = wave; j < cl; j += kPairBwdWaves) {
        const Row y = load_row(cdoc + (size_t)j * kD, lane);
        const float b_j = wb[j], g_j = gt[j], v_j = v[j];
        const int is = istar[j];
        Row acc = zero;
#pragma unroll 2
        for (int i = 0; i < ql; ++i) {
            const float d = dist[i * ld + j], C = fmaxf(d, 1e-4f);
            const float V = expf(la[i] + (f[i] - (C - c0) + g_j) / eb);
            const float M = (jstar[i] == j ? u[i] : 0.f) + (i == is ? v_j : 0.f);
            const float w = (d > 0.f ? M / d : 0.f) - (d > 1e-4f ? b_j * V / C : 0.f);
            add_diff(acc, w, load_row(qdoc + (size_t)i * kD, lane), y);
        }
        store_row(gc + (size_t)j * kD, lane, scaled(gs, acc));
    }
    zero_pad_rows(fr, lane, wave);
}

}  // namespace

// One workgroup per pair of `q` / `c` (PAIRED: q.n == c.n); rows_q / rows_c: host-known bounds of the documents' rows
// (<= generic_max_rows()).  grad_q / grad_c are laid out like q.rows / c.rows.
int launch_ot_backward(const RepSet& q, const RepSet& c, const aspire_ot_params* prm, const float* diameter, int64_t diam_group, int want,
                       const float* grad_scores, float* grad_q, float* grad_c, int rows_q, int rows_c, hipStream_t stream) {
    // the LDS layout below is int arithmetic on the rows, so they are checked before it is formed; launch_pair_bwd asks again,
    // deliberately redundant (the other launchers form their sizes in size_t and leave the check to it)
    if (int rc = check_row_bounds(rows_q, rows_c)) return rc;
    ASPIRE_REQUIRE(generic_max_rows() <= kOtBwdSide, ASPIRE_ERR_UNSUPPORTED, "the OT backward holds one row or column per thread of a half workgroup");
    const size_t lds_bytes = (size_t)ot_bwd_layout(rows_q, rows_c).total * sizeof(float);
    OtBwdArgs a{q, c, (float)prm->blur, (float)prm->sent_sm_temp, log(prm->blur), log(prm->scaling), diameter, diameter ? diam_group : 1,
                want, grad_scores, grad_q, grad_c};
    return launch_pair_bwd(ot_bwd_kernel, a, c.n, lds_bytes, 96 * 1024, rows_q, rows_c, stream);
}

}  // namespace aspire
