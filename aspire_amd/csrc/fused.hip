// otAspire throughput kernel: pairwise sentence costs AND the Sinkhorn solve of a pair in ONE launch, nothing handed over
// through HBM (A5-A8; reference arithmetic: src/learning/facetid_models/pair_distances.py:21-92 + geomloss 0.2.4's
// sinkhorn_tensorized, restated -- see sinkhorn.hip).
//
// Why fused.  For few queries per candidate the cost stage is HBM bound (24.6 KB of candidate rows per pair, 98 K flop)
// and the Sinkhorn stage is VALU / transcendental bound (~80 epsilon steps on an 8 x 8 problem).  As two kernels they
// run one after the other (1 x 20 000: 110 + 50 us), and running them side by side on two streams costs more in
// cross-stream waits than it hides (measured: 20 jobs x 1000 candidates 169 us on one stream, 213 / 266 / 403 us in 2 / 4 /
// 8 chunks over two streams).  Here a wave that has finished the costs of its four candidates solves those four pairs at
// once from its own registers while the other resident waves keep the memory system busy: the solve costs issue slots the
// streaming phase leaves idle, and the 516 B / pair workspace round trip disappears.
//
// Work decomposition (gfx950, wave = 64 lanes), documents of <= 8 sentence rows, CSR inputs:
//   * item = four consecutive candidates of ONE query (groups never straddle two jobs of a batch); a wave owns an item and
//     walks the items with a static stride (SELF: a run of consecutive items).  (Claiming items dynamically -- one atomicAdd
//     on a shared counter per item -- was measured and dropped: 2048 waves finishing an item together queue 2048
//     same-address atomics, ~40 us per round; and it buys nothing here: the kernel is bandwidth bound, so a last partial
//     round of fewer waves simply runs each of them faster.)
//   * cost phase: 16 lanes per candidate stage its 8 rows 64 coordinates at a time (coalesced global_load_dwordx4 ->
//     ds_write_b128 into padded rows), the row norms and the bounding-box term (geomloss's diameter) fall out of the
//     registers before they go to LDS, the NEXT stage's loads then go out into the same registers; the dot products run on
//     the matrix pipe (v_mfma_f32_4x4x1: 16 blocks of 4 x 4 = the 64 entries of each of the wave's four pairs; conflict-free
//     ds_read_b128 operands) and are transposed through LDS into the solve's layout: lane (li, lj) of a candidate's 16
//     lanes owns the 2 x 2 entries (2 li + x, 2 lj + y).
//   * solve phase: the same 16 lanes x (2 x 2) layout IS a Sinkhorn layout: row sums are two quad_perm DPP adds, column sums
//     two row_ror DPP adds, both inside a DPP row of 16 lanes; four solves per wave, every pair on its own epsilon schedule
//     (the loop runs to the longest of the four, finished pairs idle with h = 0).  One exponential per entry and step,
//     K_ij = 2^((f_i + g_j - C_ij) log2e / eps), weights as plain factors, f_i -= h log2(sum_j b_j K_ij) (see
//     sinkhorn_block_kernel in sinkhorn.hip for the derivation).  A sum that leaves fp32 range (extreme scaling, never at the
//     reference's hyper-parameters) poisons the pair's score with NaN; with such hyper-parameters the launcher follows up
//     with the long-form kernel (generic.hip: max-shifted log-sum-exps), which re-solves exactly the NaN pairs.
//   * Solve16 (pair_solve16_kernel; fused_solve.h): with calls in flight on several streams a batch of <= 64 jobs is cut into
//     super-items of sixteen consecutive candidates of one job instead; a wave streams its super-item as four items (the same
//     stage loop and epilogue: a pair's costs and diameter are the same bits), carries no solve through its stages, and solves the
//     sixteen pairs in one piece in a four-lanes-per-pair layout that reproduces the 16-lane sums bit for bit at 102 issue slots
//     per epsilon step for sixteen pairs against 4 x 31.  The solve tail of one call runs under the streaming of the next:
//     20 x 1000 pairs, three calls in flight, on one box 99.9 -> 92.3 us per call (cost phase alone: 72.5 us); one call at a
//     time it loses 22 % and is not taken (solve16_wanted below; NOTES.md, "Solve16").
#include <math.h>

#include <atomic>
#include <mutex>

#include "common.h"
#include "score_device.h"
#include "score_types.h"
#include "exact_d2.h"
#include "fused_solve.h"
#include "tuning.h"

namespace aspire {
namespace {

#ifdef ASPIRE_PHASE_CLOCK
// debug build only (tools/chunkphases.py): per-wave time stamps (100 MHz wall clock) into the buffer set by
// aspire_debug_fused_buffer: [wave][8] = start, then per item (end of its streaming phase, its solve set up), ..., [6] the
// wave's last solve begins, [7] end
static __device__ long long* g_fdbg = nullptr;
#define F_STAMP(k)                                                                                                   \
    do {                                                                                                             \
        if (g_fdbg && lane == 0 && (k) < 8) g_fdbg[(size_t)(blockIdx.x * 4 + wave) * 8 + (k)] = (long long)__builtin_amdgcn_s_memrealtime(); \
    } while (0)
#else
#define F_STAMP(k) \
    do {           \
    } while (0)
#endif


// MFMA: the dot products on the matrix pipe (v_mfma_f32_4x4x1_16B_f32: 16 blocks of 4 x 4 = the 64 entries of each of the
// wave's four pairs, one coordinate per instruction, exact fp32 multiply-adds), which leaves the VALU issue slots to the
// staging side products and to the solve slices -- with two waves per SIMD the kernel is otherwise VALU-issue bound
// (20 x 1000 pairs: 146 -> 130 us; 100 x 1000: 661 -> 566 us).  !MFMA: the same sums as VALU FMAs (kept for A/B and parity
// tests).  SOLVE = false (diagnostics): the cost phase alone, diam^2 as the score.
// SELF (batches of <= 64 jobs): no tables, no query boxes from a launch in front of this one -- every wave derives an item's
// documents from job_off itself (a 64-lane scan, once) and forms the query's box per stage from the query rows it has just
// staged (+32 min/max and 8 LDS reads per stage, against ~7 us for the extra launch in a 115 us call).
// L2MAX (with SOLVE = false): tsAspire on the same streaming phase -- the score is the maximum of -cdist over the valid
// block (allpair_masked_dist_l2max, pair_distances.py:167-176); no boxes, no solve.
// QBOX (one query against a big pool): the in-wave query box of SELF without its tables -- every item has the same query, so
// the box is formed during a wave's first item and read from the LDS cache afterwards; no doc_box launch in front.
// CHUNK (batched jobs whose candidates reach 9 .. 32 rows, queries of <= 8: config 4's facet-selected queries against whole
// abstracts -- pp_settings.py:2-3, models.py:127-163): an item's four 16-lane groups hold four 8-row CHUNKS instead of four
// candidates -- four candidates of <= 8 rows, two of 9 .. 16 (two chunks each) or one of 17 .. 32 (four); chunk_prep_kernel
// (batch_prep.hip) sorts a job's candidates into such items.  The streaming phase is the same (a group stages rows row0 .. row0 + 7
// of its document; the candidate's per-coordinate box is joined across its groups), the solve's row sums and the marginals'
// normalisations cross the candidate's groups (xg_sum / xg_max).
// (-DASPIRE_FUSED_WAVES3: the experiment of NOTES.md -- the same kernel built for three workgroups per CU, 168 registers: the
// compiler spills the kernel-invariant values and the launch gets slower; profiles/r03_fused_3waves_* hold its counters)
#ifndef ASPIRE_FUSED_MFMA_UNROLL
#define ASPIRE_FUSED_MFMA_UNROLL 4
#endif
constexpr int kMfmaUnroll = ASPIRE_FUSED_MFMA_UNROLL;      // coordinates chunks per iteration of a stage's MFMA loop
#ifdef ASPIRE_FUSED_WAVES3
#define ASPIRE_FUSED_MIN_WAVES 3
#else
#define ASPIRE_FUSED_MIN_WAVES 2
#endif
template <bool MFMA, bool SOLVE = true, bool SELF = false, bool L2MAX = false, bool QBOX = false, bool CHUNK = false>
__global__ void __launch_bounds__(256, ASPIRE_FUSED_MIN_WAVES) pair_fused_kernel(ScoreArgs a, const float* __restrict__ qbox) {
    constexpr bool S16 = false;
#include "fused_kernel_body.h"
}
// S16 (an option of the SELF form; fused_solve.h, Solve16): an item is one of the four sub-items of a super-item, sixteen consecutive
// candidates of one job; a wave streams a super-item and then solves its sixteen pairs in one piece in the four-lanes-per-pair
// layout -- fewer issue slots per pair and step, no solve slices inside the stages.  Same bits as the other forms.
__global__ void __launch_bounds__(256, ASPIRE_FUSED_MIN_WAVES) pair_solve16_kernel(ScoreArgs a, const float* __restrict__ qbox) {
    constexpr bool MFMA = true, SOLVE = true, SELF = true, L2MAX = false, QBOX = false, CHUNK = false, S16 = true;
#include "fused_kernel_body.h"
}

}  // namespace

// (when a call takes which form of the kernel: forms.hip -- fused_path_ok, fused_self_ok, fused_inbox_ok)
// tsAspire (max-sim) of every (query, candidate) pair, CROSS, documents of <= 8 rows: the fused kernel's streaming phase
// self (batched jobs, <= 64 of them): no tables in front of the launch -- the waves derive an item's job from job_off (SELF)
int launch_pair_fused_l2max(const ScoreArgs& a, int64_t groups_bound, hipStream_t stream, bool self) {
    const int64_t cap = tuning().fused_waves > 0 ? tuning().fused_waves : 256 * 8;
    const int64_t waves = groups_bound < cap ? groups_bound : cap;
    const dim3 grid((unsigned)((waves + 3) / 4));
    if (self)
        hipLaunchKernelGGL((pair_fused_kernel<true, false, true, true>), grid, dim3(256), 4 * kWaveLds * sizeof(float), stream, a,
                           (const float*)nullptr);
    else
        hipLaunchKernelGGL((pair_fused_kernel<true, false, false, true>), grid, dim3(256), 4 * kWaveLds * sizeof(float), stream, a,
                           (const float*)nullptr);
    ASPIRE_LAUNCH_OK();
    return ASPIRE_OK;
}

// The SELF form's Solve16 option (pair_solve16_kernel).  Its waves solve in one piece behind their streaming, so a launch
// that has the chip to itself ends in ~25 us of solves with nothing streaming beside them (20 x 1000 pairs, one call at a time:
// 184.5 -> 143.8 M alignments/s), while with calls in flight on several streams the next call's streaming fills that tail and the
// cheaper solve shows (one box, six runs each: 199 - 201 -> 216 - 217 M; NOTES.md).  Either form gives the same bits, so the
// choice is one of speed alone.  ASPIRE_HIP_FUSED_SOLVE16 / aspire_debug_set("FUSED_SOLVE16", "0" | "1") is the caller's explicit
// word.  Unpinned, the library guesses: it sees no queue depth, but it sees streams -- callers that keep calls in flight
// rotate them (scorer.InFlightRanker, bench.py), a caller that waits for each call usually stays on one -- and a launch takes
// the form when its stream differs from the previous SELF launch's (one word of process-wide state).  Where the guess is WRONG,
// and the pin is the answer: a caller that takes a fresh or alternating stream per request but waits for each call, and one
// process that walks several devices in turn with a stream each, get Solve16 with nothing to overlap it (the 22 % above);
// threads that each stay on their own stream look like one rotating caller (which they are, if their calls overlap); the
// first launch after a change of stream is judged by the launch before it, whoever made that.
static std::atomic<long long> g_solve16_launches{0};
static bool solve16_wanted(hipStream_t stream) {
    static std::atomic<uintptr_t> last{1};      // 1: no launch yet (no stream handle is odd)
    const uintptr_t prev = last.exchange((uintptr_t)stream);
    const bool rotating = prev != 1 && prev != (uintptr_t)stream;
    return tuning().fused_solve16 < 0 ? rotating : tuning().fused_solve16 == 1;
}
}  // namespace aspire
long long aspire::solve16_launches() { return g_solve16_launches.load(); }
namespace aspire {

// groups_bound: upper bound of the launch's items (groups of four candidates x queries)
int launch_pair_fused(const ScoreArgs& a_in, int64_t groups_bound, const float* qbox, hipStream_t stream) {
    // two 4-wave workgroups per CU are resident.  (Built for three -- 168 registers, the kernel-invariant values spilled,
    // the norm table already shares the stage buffer so the LDS fits -- the 20 x 1000 call went from 120 to 144 us.)
    ScoreArgs a = a_in;
    a.skip_tail = tuning().fused_nosolve == 2;
    a.no_repair = tuning().fused_norepair == 1;
    const int64_t cap = tuning().fused_waves > 0 ? tuning().fused_waves : 256 * 8;
    const int64_t waves = groups_bound < cap ? groups_bound : cap;
    const dim3 grid((unsigned)((waves + 3) / 4));
    const bool self = qbox == nullptr && a.pairing == kPairMapped;       // batched jobs without the tables launch (fused_self_ok)
    const bool inbox1 = qbox == nullptr && a.pairing == ASPIRE_PAIR_CROSS;      // one query, box in-wave (fused_inbox_ok)
    if ((self || inbox1) && (tuning().fused_nosolve == 1 || tuning().fused_valu)) return ASPIRE_ERR_INVALID_ARG;
    const size_t lds = 4 * (kWaveLds + (self || inbox1 ? 2 * kD : 0)) * sizeof(float);      // + a query-box cache per wave
    if (tuning().fused_nosolve == 1) hipLaunchKernelGGL((pair_fused_kernel<true, false>), grid, dim3(256), lds, stream, a, qbox);
    else if (tuning().fused_valu) hipLaunchKernelGGL((pair_fused_kernel<false, true>), grid, dim3(256), lds, stream, a, qbox);
    else if (self && tuning().fused_nosolve == 0 && solve16_wanted(stream)) {
        // the Solve16 form: one wave per super-item of sixteen candidates (at most ceil(groups / 4) + one partial per job of them)
        const int64_t supers = (groups_bound + 3) / 4 + (a.job1 - a.job0);
        const int64_t waves16 = supers < cap ? supers : cap;
        static std::once_flag raised16;
        static hipError_t raise16_rc = hipSuccess;
        std::call_once(raised16, [] {
            raise16_rc = hipFuncSetAttribute(reinterpret_cast<const void*>(pair_solve16_kernel),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, 80 * 1024);
        });
        ASPIRE_HIP_OK(raise16_rc);
        ++g_solve16_launches;
        hipLaunchKernelGGL(pair_solve16_kernel, dim3((unsigned)((waves16 + 3) / 4)), dim3(256), lds,
                           stream, a, qbox);
    }
    else if (self) {
        // 67.6 KB of dynamic LDS: above the default limit of 64 KB (raised once per process; two workgroups still fit a CU)
        static std::once_flag raised;
        static hipError_t raise_rc = hipSuccess;
        std::call_once(raised, [] {
            raise_rc = hipFuncSetAttribute(reinterpret_cast<const void*>(pair_fused_kernel<true, true, true>),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, 80 * 1024);
        });
        ASPIRE_HIP_OK(raise_rc);
        hipLaunchKernelGGL((pair_fused_kernel<true, true, true>), grid, dim3(256), lds, stream, a, qbox);
    }
    else if (inbox1) {
        static std::once_flag raised1;
        static hipError_t raise1_rc = hipSuccess;
        std::call_once(raised1, [] {
            raise1_rc = hipFuncSetAttribute(reinterpret_cast<const void*>(pair_fused_kernel<true, true, false, false, true>),
                                            hipFuncAttributeMaxDynamicSharedMemorySize, 80 * 1024);
        });
        ASPIRE_HIP_OK(raise1_rc);
        hipLaunchKernelGGL((pair_fused_kernel<true, true, false, false, true>), grid, dim3(256), lds, stream, a, qbox);
    }
    else hipLaunchKernelGGL((pair_fused_kernel<true, true>), grid, dim3(256), lds, stream, a, qbox);
    ASPIRE_LAUNCH_OK();
    return ASPIRE_OK;
}

}  // namespace aspire
#ifdef ASPIRE_PHASE_CLOCK
extern "C" void aspire_debug_fused_buffer(void* p) {
    long long* q = (long long*)p;
    (void)hipMemcpyToSymbol(HIP_SYMBOL(aspire::g_fdbg), &q, sizeof(q));
}
#endif
namespace aspire {
// tsAspire on the same items: the streaming phase with the max epilogue
int launch_pair_fused_chunk_l2max(const ScoreArgs& a, int64_t items_bound, hipStream_t stream) {
    const int64_t cap = tuning().fused_waves > 0 ? tuning().fused_waves : 256 * 8;
    const int64_t waves = items_bound < cap ? items_bound : cap;
    hipLaunchKernelGGL((pair_fused_kernel<true, false, false, true, false, true>), dim3((unsigned)((waves + 3) / 4)), dim3(256),
                       4 * kWaveLds * sizeof(float), stream, a, (const float*)nullptr);
    ASPIRE_LAUNCH_OK();
    return ASPIRE_OK;
}

// batched jobs with candidates of up to 32 rows against queries of <= 8 (the CHUNK form; items from chunk_prep_kernel)
int launch_pair_fused_chunk(const ScoreArgs& a_in, int64_t items_bound, const float* qbox, hipStream_t stream) {
    ScoreArgs a = a_in;
    a.skip_tail = tuning().fused_nosolve == 2;
    a.no_repair = tuning().fused_norepair == 1;
    const int64_t cap = tuning().fused_waves > 0 ? tuning().fused_waves : 256 * 8;
    const int64_t waves = items_bound < cap ? items_bound : cap;
    const dim3 grid((unsigned)((waves + 3) / 4));
    if (tuning().fused_nosolve == 1)      // timing experiments: the streaming phase alone
        hipLaunchKernelGGL((pair_fused_kernel<true, false, false, false, false, true>), grid, dim3(256), 4 * kWaveLds * sizeof(float), stream, a, qbox);
    else
        hipLaunchKernelGGL((pair_fused_kernel<true, true, false, false, false, true>), grid, dim3(256), 4 * kWaveLds * sizeof(float), stream, a, qbox);
    ASPIRE_LAUNCH_OK();
    return ASPIRE_OK;
}

}  // namespace aspire
