// Which kernel family scores a call (forms.h).  No kernel and no launch here: every rule that picks a family, every threshold with
// its measurement, and the order in which the rules are tried -- planes, the one-query 16-row stream, Gram, fused, long documents.
// A family decides a pair's bits, so a rule two entry points ask is one function called twice; tuning()'s form switches (OT_FORM,
// COST_PATH, SINKHORN, FUSED_NOSELF and FUSED_VALU / FUSED_NOSOLVE / GEMM as form exclusions) are read here and nowhere else.
#include "forms.h"

#include "common.h"
#include "tuning.h"
#include "score_types.h"

namespace aspire {
static_assert(kTileMaxRows == 8 * kMaxT, "the tile kernels' row bound");
namespace {

// ---- thresholds ---------------------------------------------------------------------------------------------------------------
// groups (waves' worth of items) that fill the chip: 256 CUs x 8 resident waves.  From here the throughput kernels' grids are full
// (the tiled cost kernel: 4.7 TB/s algorithmic at 1 x 20 000 against 1.8 TB/s for the accumulate-then-reduce kernel).
constexpr int64_t kChipGroups = 256 * 8;
// Groups of four candidates from which the fused streaming kernel (fused.hip) is ahead of the small-pool kernels, documents of
// <= 8 rows (tools/otbatchcross.py: one query x one pool 750 groups 39 against 46 us, 2000 groups 59 / 94; batched jobs 500
// groups 33 / 37, 1600 groups 45 / 79).  Below, a call is latency bound and the small-pool kernels' shorter chains win.
constexpr int64_t kStreamMinGroups1 = 640, kStreamMinGroupsBatch = 512;
// groups of four candidates from which batched max-sim takes the streaming kernels (measured, tools/l2batchbench.py)
constexpr int64_t kL2StreamMinGroups = 384;
// ONE query against documents of 9 .. 16 rows: candidates from which the 16-row streaming kernel fills the chip (two per wave)
constexpr int64_t kStream16MinCands = 2 * kChipGroups;
// smallest pool / batch (candidates) that takes the CHUNK / REC forms (below: the small-batch kernels; tools/csfbench.py sweeps)
constexpr int64_t kChunkMinCands = 256;
// pairs of short documents per call that take pair_one_kernel (tools/experiments/singlejob.py sweeps)
constexpr int64_t kOneMinPairs = 1, kOneMaxPairs = 8192;        // (ONE form for every small grid: a pair scored alone, in a subset or in a shard gets the same bits)
// candidates of a batch from which the hybrid forms pay (the census + the fused launch in front of the 16-row kernels)
constexpr int64_t kHybridMinCands = 6000;
// jobs the fused kernel's waves derive the tables for themselves (one lane per job)
constexpr int64_t kSelfMaxJobs = 64;
// the in-wave re-solve of overflowed sums stays the exception from this scaling on (fused.hip, solve_safe)
constexpr double kFusedMinScaling = 0.25;
// Gram tiles (gram_path_wanted): candidate tiles from which the pool fills the chip / long documents pay the kernel's latency
constexpr int64_t kGramMinTiles = 128, kGramMinTilesLong = 32, kGramMinWorkLong = 16000, kGramMinQueryRows = 24;
// pairs of CSR documents of more than 8 rows below which every 8 x 8 sub-tile is an item of the small-pool kernel (1 x 125 x 20:
// 125 workgroups walking 9 tiles each -> 1024 side by side, 54 -> 36 us; from ~1000 pairs the per-pair kernel is ahead again)
constexpr int64_t kSubTileMaxPairs = 512;
// The solve stage.  One solve per wave has the lowest latency (15.4 vs 26.7 us per call at 50 pairs), the block forms several
// times the throughput; measured crossovers (1 x N x 8, cost + solve, us): N = 5000: wave 58 / 16-lane block 64 / 4-lane block 68;
// 8000: 88 / 83 / 89; 12000: 119 / 109 / 106.  S = 12 / 20: even at 2000 / ~2500, block ahead at 3000.
constexpr int64_t kBlock16MinSlots = 7000, kBlockMinSlots = 10000, kBlockMinSlotsLong = 2500;
// The dense layouts (documents of <= 8 rows: ONE lane per pair, 8 x 8 entries, no cross-lane step at all; 9 .. 16 rows: 2 x 2
// lanes of 6 x 6 / 8 x 8 entries) need a third fewer issue slots per pair than the wide ones (2 x 2 lanes of 4 x 4; 4 x 4 lanes of
// 3 x 3 / 4 x 4): 32 x 50 000 x 8 0.90 -> 0.74 ms per launch, 128 x 8192 x 12 1.10 -> 0.76, x 16 1.59 -> 1.27 -- but hold 64 / 16
// pairs per wave, so only grids that still fill the chip take them.
constexpr int64_t kDenseMinSlots = 196608, kDenseMinSlotsLong = 49152;

bool chip_filling(int64_t groups) { return groups >= kChipGroups; }
bool csr(const aspire_repset* q, const aspire_repset* c) { return q->ext == 0 && c->ext == 0; }

// ---- rules asked by more than one family ----------------------------------------------------------------------------------------
// documents of <= 8 rows on the fused kernel's streaming phase: pinned (OT_FORM=fused), or by default from `min_groups` groups of four
bool stream_short(int64_t groups4, int64_t min_groups) {
    const int form_t = tuning().ot_form;
    return form_t == 3 || (form_t == 0 && groups4 >= min_groups);
}
// ... of a single-pool call: ONE query from kStreamMinGroups1, several once the tiled cost kernel's grid would be full
int64_t stream_min_groups_call(const aspire_repset* q) { return q->n == 1 ? kStreamMinGroups1 : kChipGroups; }

// fused.hip serves CSR documents of <= 8 rows
bool fused_path_ok(const aspire_repset* q, const aspire_repset* c) {
    const int mq = q->max_len, mc = c->max_len;
    return csr(q, c) && mq > 0 && mc > 0 && mq <= 8 && mc <= 8;
}
// tile16.hip: documents of 9 .. 16 rows (both sides), CSR, CROSS or MAPPED pairing with the job tables built
bool tile16_path_ok(const aspire_repset* q, const aspire_repset* c, int pairing) {
    if (!csr(q, c) || (pairing != ASPIRE_PAIR_CROSS && pairing != kPairMapped)) return false;
    const int mq = q->max_len, mc = c->max_len;
    return mq > 0 && mc > 0 && mq <= 16 && mc <= 16 && (mq > 8 || mc > 8);
}
// ONE query against a big pool of 9 .. 16-row documents: the streaming kernel (tile16.hip) beats the 32-column Gram tiles, whose
// 12 .. 16 real query rows fill a third to a half of the MFMA tile (1 x 20 000 x 12 otAspire: 247 vs 363 us; at two queries they
// tie, from three the Gram tiles win: 623 vs 565 us)
bool stream16_one_query(const aspire_repset* q, const aspire_repset* c, int pairing) {
    return q->n == 1 && c->n >= kStream16MinCands && tile16_path_ok(q, c, pairing) && tuning().cost_path != 1 && tuning().ot_form != 1;
}
// the fused kernel's forms that solve inside the stage loop (SELF, QBOX) are built as <MFMA, SOLVE> only (launch_pair_fused's guard)
bool fused_in_wave_solve_ok() { return tuning().fused_nosolve != 1 && !tuning().fused_valu; }
// batched jobs: few enough jobs for the in-wave tables, and hyper-parameters at which overflowed sums stay the exception
bool fused_self_ok(int64_t jobs, const aspire_ot_params* prm) {
    return jobs <= kSelfMaxJobs && prm->scaling >= kFusedMinScaling && fused_in_wave_solve_ok() && !tuning().fused_noself;
}
// one query against a pool with its own per-pair diameters: the box comes from the staged query rows (no box launch).
// REVIEW: unlike fused_self_ok this asks no scaling >= kFusedMinScaling; nothing records why.  Kept as it is.
bool fused_inbox_ok(const aspire_repset* q, bool caller_diameters) {
    return q->n == 1 && !caller_diameters && fused_in_wave_solve_ok() && !tuning().fused_noself;
}
// the size rule of the CHUNK / REC forms: pinned (OT_FORM=chunk), or by default from kChunkMinCands candidates in the call
bool chunk_size_ok(int64_t C) {
    const int form_t = tuning().ot_form;
    return form_t == 4 || (form_t == 0 && C >= kChunkMinCands);
}
// May a call of `pairs` pairs of documents of <= 8 rows take the one-launch form (pair_one_kernel: one wave per pair, costs and
// solve)?  The single-pool and the batched entry points ask the same question, so that a pair gets the same kernel -- the same
// bits -- whether it is scored in a call of its own or in a batch.
//   plain_call: CSR sets, no Gram tiles, every stage of the call wanted.  Single-pool: ext == 0 on both sides && !gram &&
//               !cost_only; batched: the full stage mask (batched sets are CSR and never take the Gram tiles).
//   small_grid: the call stays below the throughput kernels.  The two callers' rules differ and stay their own: single-pool calls
//               go by groups of four (CROSS pairing from kChipGroups groups: the tiled cost kernel's grid), batches by !tile_form
//               (from kStreamMinGroupsBatch groups the fused kernel, which also carries the OT_FORM pins 2 and 3).
bool one_wave_form_ok(int64_t pairs, bool plain_call, bool small_grid) {
    const int form_t = tuning().ot_form;
    return plain_call && small_grid && pairs >= kOneMinPairs && pairs <= kOneMaxPairs &&
           (form_t == 5 || (form_t == 0 && tuning().sinkhorn_form == 0 && tuning().cost_path == 0 && tuning().cost1_blocks == 0));
}
// The hybrid forms (fused kernel in front of the 16-row kernels, ScoreArgs::gate) need a solve stage that leaves the short pairs'
// scores alone: the block kernels and their repair kernel check the gate, the one-solve-per-wave kernel (SINKHORN=wave) does not.
bool sinkhorn_form_honours_gate() {
    const int f = tuning().sinkhorn_form;
    return f == 0 || f == 3 || f == 5 || f == 6 || f == 7;
}
// a batch big enough for the hybrid forms
bool hybrid_size_ok(int64_t groups_bound, int64_t C) { return chip_filling(groups_bound) && C >= kHybridMinCands; }

int64_t gram_cand_tiles(const aspire_repset* c) {
    const int per_tile = kGramCandRows / gram_slot_rows(c->max_len);
    return (c->n + per_tile - 1) / per_tile;
}
// Max-sim on the fp16-plane tiles whatever the number of queries: both rep sets carry planes around one centre, the pool fills the
// chip (>= 128 candidate tiles), and it is not the one case the streaming kernel wins (ONE query of <= 8 rows against documents of
// <= 8: the fused kernel's max-sim form reads each row once at 6 TB/s and has no wasted columns -- 81 against 95 us at 1 x 20 000 x 8)
bool gram_planes_wanted_l2max(const aspire_repset* q, const aspire_repset* c, int pairing) {
    if (pairing != ASPIRE_PAIR_CROSS || !csr(q, c) || !q->planes || !c->planes) return false;
    if (q->max_len <= 0 || c->max_len <= 0 || q->max_len > kTileMaxRows || c->max_len > kTileMaxRows) return false;
    if (tuning().cost_path == 2 || tuning().gemm_form == 1 || tuning().gemm_form == 2) return false;
    if (q->planes->mu != c->planes->mu || !q->planes->planes || !c->planes->planes) return false;
    if (gram_cand_tiles(c) < kGramMinTiles) return false;
    return !(q->n == 1 && q->max_len <= 8 && c->max_len <= 8);
}
// otAspire's cost stage on the plane tiles with FEW queries too: as above, and the pairs' diameters must not cost a pass over every
// candidate row -- the pool brings its documents' boxes along (aspire_repset.doc_box) or the caller its own diameters.  Two to eight
// queries against 20 000 documents of 8 rows then take cost tiles (~90 us) + pair_box + the block Sinkhorn kernel instead of the
// fused kernel re-staging every candidate group per query (Q = 4: 335 us, Q = 8: 626).  ONE query of <= 8 rows stays on the fused /
// chunk kernels.
bool gram_planes_wanted_ot(const aspire_repset* q, const aspire_repset* c, int pairing, bool caller_diameters) {
    if (!gram_planes_wanted_l2max(q, c, pairing)) return false;
    if (!c->doc_box && !caller_diameters) return false;
    return !(q->n == 1 && q->max_len <= 8);
}
}  // namespace

int max_rows_of(const aspire_repset* q, const aspire_repset* c) {
    const int mq = q->ext > 0 ? q->ext : q->max_len;
    const int mc = c->ext > 0 ? c->ext : c->max_len;
    return mq > mc ? mq : mc;
}

int gram_slot_rows(int max_len) {
    const int r = (max_len + 3) / 4 * 4;
    return r < 8 ? 8 : r;
}

// The matrix-core form serves CSR inputs (no padded extents) scored all-against-all, once the query side fills
// a useful part of an MFMA tile or documents are longer than the 8-row VALU tile.
bool gram_path_wanted(const aspire_repset* q, const aspire_repset* c, int pairing) {
    if (pairing != ASPIRE_PAIR_CROSS || !csr(q, c)) return false;
    if (q->max_len <= 0 || c->max_len <= 0 || q->max_len > kTileMaxRows || c->max_len > kTileMaxRows) return false;
    // ASPIRE_HIP_COST_PATH=mfma|valu pins the choice (parity tests compare the two forms); default: by shape
    if (tuning().cost_path == 1) return true;
    if (tuning().cost_path == 2) return false;
    const int max_rows = q->max_len > c->max_len ? q->max_len : c->max_len;
    const int64_t tiles = gram_cand_tiles(c);
    if (max_rows > 8) {
        // long documents: the VALU tile-loop kernel costs ~5 ns per (pair x 8x8 tile), the Gram kernel ~75 us of
        // latency (48 dependent K stages) before its throughput counts: 1 x 3000 x 12 is 82 vs 88 us, 1 x 4000 x 20
        // 194 vs 120 us
        const int64_t T = (max_rows + 7) / 8;
        return tiles >= kGramMinTilesLong && q->n * c->n * T * T >= kGramMinWorkLong;
    }
    if (tiles < kGramMinTiles) return false;          // small pools are latency bound: the per-pair kernels start faster
    return q->n * (int64_t)gram_slot_rows(q->max_len) >= kGramMinQueryRows;
}

// ---- max-sim per call ---------------------------------------------------------------------------------------------------------
ScorePlan plan_l2agg(const aspire_repset* q, const aspire_repset* c, int pairing, int agg, bool pair_outputs, bool one_form) {
    ScorePlan p{};
    p.max_rows = max_rows_of(q, c);
    const bool maxsim = agg == ASPIRE_AGG_MAX && !pair_outputs;      // the other aggregations and the pair outputs: the VALU tiles only
    const bool long_docs = p.max_rows > kTileMaxRows;
    if (one_form) p.form = Form::Generic;      // every pair through the long-form kernel, whatever the size of the call
    // both sides carry fp16 planes: the matrix-pipe tiles (gramp.hip) whatever the number of queries
    else if (maxsim && gram_planes_wanted_l2max(q, c, pairing)) p.form = Form::GramPlanes;
    else if (maxsim && stream16_one_query(q, c, pairing)) p.form = Form::Stream16;
    else if (maxsim && gram_path_wanted(q, c, pairing)) p.form = Form::Gram;
    // Few queries against a big pool of short documents (CSR): the fused kernel's streaming phase with a max epilogue --
    // four candidates per wave, dot products on the matrix pipe (l2max_kernel<1> is one workgroup per candidate with VALU
    // difference sums: 114 us at 1 x 20 000 against the stream's 88)
    else if (maxsim && pairing == ASPIRE_PAIR_CROSS && fused_path_ok(q, c) &&
             stream_short((c->n + 3) / 4 * q->n, stream_min_groups_call(q))) p.form = Form::FusedStream;
    // Documents beyond the tile kernels' 32 rows: padded tensors that wide go through the one-workgroup-per-pair kernel for every
    // pair; CSR pools run the tile kernel on 32-row tiles first (it covers every pair of short documents) and the long-document
    // kernel then rewrites the pairs that hold a longer one.
    else if (long_docs && !csr(q, c)) p.form = Form::Generic;
    else {
        p.form = Form::Tiles;
        p.then_generic = long_docs;
        if (long_docs) p.max_rows = kTileMaxRows;
    }
    return p;
}

// ---- otAspire per call --------------------------------------------------------------------------------------------------------
namespace {
// the forms of documents of up to 32 rows (q / c carry the clamped row bound)
ScorePlan plan_ot_tiles(const aspire_repset* q, const aspire_repset* c, int pairing, const aspire_ot_params* prm, const OtAsked& asked) {
    ScorePlan p{};
    p.max_rows = max_rows_of(q, c);
    const bool extra = asked.pair_outputs, diameters = asked.caller_diameters, cost_only = asked.cost_only;
    // both sides on fp16 planes, the pool's boxes cached: the plane tiles whatever the number of queries (gram.hip)
    const bool planes_ot = !extra && gram_planes_wanted_ot(q, c, pairing, diameters) && tuning().ot_form == 0;
    const bool stream16 = !planes_ot && stream16_one_query(q, c, pairing);
    // ONE short query (facet-selected rows) against a pool of abstracts of up to 32 rows: the fused kernel's CHUNK form, as in
    // plan_ot_batch (1 x 20 000 x (3..20): 674 us on the Gram tiles + block Sinkhorn before) -- the item records and their counter
    // take the (unused) front of the pair-slot workspace.  (From kChunkMinCands candidates even where the form is pinned: the
    // call's workspace is sized for the pair slots.)
    // REVIEW against plan_ot_batch's `chunked`: this rule also excludes FUSED_NOSOLVE and every COST_PATH pin; the launcher serves
    // FUSED_NOSOLVE=1 on CHUNK items and the batched rule lets it through.  Nothing records that the difference is meant: kept.
    const bool chunk1 = pairing == ASPIRE_PAIR_CROSS && q->n == 1 && csr(q, c) && q->max_len <= 8 && c->max_len > 8 &&
                        c->max_len <= kTileMaxRows && c->n >= kChunkMinCands && c->n < ((int64_t)1 << 30) && !extra && !cost_only &&
                        !diameters && chunk_size_ok(c->n) && prm->scaling >= kFusedMinScaling && !tuning().fused_nosolve &&
                        !tuning().fused_valu && tuning().cost_path == 0 && asked.has_workspace &&
                        (size_t)(chunk_items_bound(1, c->n, c->n) + 2) * 64 + 256 + qbox_bytes(q) + 64 <= asked.workspace_bytes;
    p.gram = (gram_path_wanted(q, c, pairing) || planes_ot) && !stream16 && !chunk1;
    // the matrix-pipe cost tiles derive -cdist and geomloss's cost from ONE distance: they store -cdist only and the solve stage takes
    // cost = max(cdist, 1e-4) from it -- half the tile bytes written and read (the debug cost stage keeps both buffers)
    p.cost_from_neg = p.gram && !cost_only;
    // Few queries against a big pool of short documents: costs and solves in ONE launch, no workspace slots, no candidate
    // chunks (fused.hip).
    if (pairing == ASPIRE_PAIR_CROSS && !extra && !p.gram && !cost_only && fused_path_ok(q, c) &&
        stream_short((c->n + 3) / 4 * q->n, stream_min_groups_call(q))) {
        p.form = fused_inbox_ok(q, diameters) ? Form::FusedInbox : Form::FusedQbox;
        p.qbox_first = p.form == Form::FusedQbox && !diameters;      // per-coordinate boxes of the queries (the kernel adds each candidate's rows)
    } else {
        p.form = chunk1 ? Form::Chunk : Form::Tiles;
    }
    return p;
}
}  // namespace

// Documents beyond the tile kernels' 32 rows: padded tensors that wide go through the one-workgroup-per-pair kernel
// (generic.hip) for every pair; CSR pools run the tile kernels with their documents' bound clamped to 32 rows (every pair
// of short documents is scored there, a pair that holds a longer one gets NaN) and the long-document kernel then rewrites
// exactly those pairs.
ScorePlan plan_ot(const aspire_repset* q, const aspire_repset* c, int pairing, const aspire_ot_params* prm, const OtAsked& asked) {
    // ONE_FORM (include/aspire_hip.h): every pair through the long-form kernel, whatever the size of the call
    const bool one_form = (prm->flags & ASPIRE_OT_FLAG_ONE_FORM) && !asked.cost_only;
    const int rows = max_rows_of(q, c);
    if (rows <= kTileMaxRows && !one_form) return plan_ot_tiles(q, c, pairing, prm, asked);
    if (csr(q, c) && !one_form) {      // (CSR: no pair outputs)
        const aspire_repset q32 = tile_bound_set(q), c32 = tile_bound_set(c);
        ScorePlan p = plan_ot_tiles(&q32, &c32, pairing, prm, asked);
        p.then_generic = !asked.cost_only;
        return p;
    }
    ScorePlan p{};
    p.form = asked.cost_only ? Form::None : Form::Generic;
    p.max_rows = rows;
    return p;
}

// a small pool of short documents (the per-query call of evaluate.py:58-76): one wave per pair, costs and solve in ONE launch
// (pair_one_kernel) instead of the cost launch + the Sinkhorn launch and the workspace between them
bool ot_chunk_one_wave(const ScorePlan& plan, const aspire_repset* q, const aspire_repset* c, int pairing, int64_t chunk_cands,
                       bool cost_only) {
    if (plan.form != Form::Tiles || plan.max_rows > 8) return false;
    const bool cross = pairing == ASPIRE_PAIR_CROSS;
    const int64_t groups4 = (chunk_cands + 3) / 4 * (cross ? q->n : 1);
    const bool small_grid = !(cross && chip_filling(groups4));        // (beyond: the tiled cost kernel's grid)
    return one_wave_form_ok(chunk_cands * (cross ? q->n : 1), csr(q, c) && !plan.gram && !cost_only, small_grid);
}

// ---- otAspire batched ---------------------------------------------------------------------------------------------------------
// Small batches are latency bound and take the kernels the single-pool entry points use.  Once the batch fills the chip (documents
// of <= 8 rows): the fused kernel -- four candidates of a job per wave, costs and solves in one launch (fused.hip) -- or, pinned
// for A/B tests, the same cost kernel + the block Sinkhorn kernel as two launches.
ScorePlan plan_ot_batch(const aspire_repset* q, const aspire_repset* c, int64_t max_job, const aspire_ot_params* prm, int want,
                        int stages) {
    ScorePlan p{};
    const int64_t J = q->n, C = c->n;
    const int max_rows_all = max_rows_of(q, c);
    const int max_rows = p.max_rows = max_rows_all < kTileMaxRows ? max_rows_all : kTileMaxRows;
    if (prm->flags & ASPIRE_OT_FLAG_ONE_FORM) {      // every pair through the long-form kernel
        p.form = (stages & kStageSolve) ? Form::Generic : Form::None;
        return p;
    }
    const int64_t groups_bound = J * ((max_job + 3) / 4);
    const int form_t = tuning().ot_form;
    const bool fused = max_rows <= 8 && stream_short(groups_bound, kStreamMinGroupsBatch);
    p.tile_form = max_rows <= 8 && (form_t == 2 || fused);
    // Short queries (facet-selected rows, models.py:127-163) against abstracts of up to 32 rows -- config 4's shape: the fused
    // kernel's CHUNK form, costs and solves of every pair in one launch behind a launch that sorts the candidates into items.
    // (FUSED_NOSOLVE passes: launch_pair_fused_chunk has the cost phase alone for timing.  REVIEW: see plan_ot_tiles' chunk1.)
    if (q->max_len <= 8 && max_rows > 8 && max_rows_all <= kTileMaxRows && chunk_size_ok(C) && stages == kStageAll &&
        prm->scaling >= kFusedMinScaling && !tuning().fused_valu) {
        p.form = Form::Chunk;
        return p;
    }
    // Whole abstracts on both sides, documents of 17 .. 32 rows among them (un-faceted queries: pp_settings.py:2-3): the 16-row
    // streaming kernel on record items (a query half against two candidate halves) + the block Sinkhorn kernel on 24- / 32-row
    // workspace slots.  (COST_PATH=valu keeps the VALU tile loop, one workgroup per candidate, for parity tests; no fused kernel
    // runs here, so its switches do not matter.)
    if (max_rows > 16 && max_rows_all <= kTileMaxRows && chunk_size_ok(C) && stages == kStageAll && tuning().cost_path != 2) {
        p.form = Form::Rec16;
        return p;
    }
    // batches of <= 64 jobs on the fused kernel need no tables launch: the kernel's waves derive them (fused.hip, SELF)
    const bool self = fused && fused_self_ok(J, prm);
    p.tables_first = (stages & kStagePrep) && !self;
    // Documents of up to 16 rows in a batch that fills the chip: usually pools of mostly short abstracts with a few longer
    // ones.  The fused kernel is queued in front of the 16-row streaming kernel + block Sinkhorn, and a census of the long
    // pairs, taken on the device, decides how they work (score_types.h: ScoreArgs::gate): few long pairs -- the fused kernel
    // scores the short ones, the 16-row kernels only the long ones; many -- the fused kernel returns at once.  No host round
    // trip, and ONE long document no longer moves 20 000 pairs onto kernels 2.5 x slower.
    // (The table-driven fused kernel runs in front, with its solve: FUSED_NOSOLVE in either value and FUSED_VALU leave the form;
    // PLAN_SIM: the fused kernel has no plan output for the 16-row kernels to complete.)
    if (max_rows > 8 && max_rows <= 16 && form_t == 0 && hybrid_size_ok(groups_bound, C) && stages == kStageAll &&
        prm->scaling >= kFusedMinScaling && want != ASPIRE_OT_PLAN_SIM && !tuning().fused_nosolve && !tuning().fused_valu &&
        sinkhorn_form_honours_gate())
        p.form = Form::Hybrid;
    else if (fused)
        p.form = !(stages & (kStageCost | kStageSolve)) ? Form::None : self ? Form::FusedSelf : Form::FusedTables;
    // a small batch of short documents: the single-pool calls' one-launch form (pair_one_kernel: one wave per pair) -- the
    // same kernel whether a pair is scored in a batch or in a call of its own: the same bits
    else if (max_rows <= 8 && one_wave_form_ok(C, stages == kStageAll, !p.tile_form))
        p.form = Form::OneWave;
    else {
        p.form = Form::Tiles;
        // documents beyond 32 rows (AspireNER's appended entity rows, models.py:224-233), as in plan_ot
        p.then_generic = max_rows_all > max_rows && (stages & kStageSolve);
    }
    return p;
}

// ---- max-sim batched ----------------------------------------------------------------------------------------------------------
// The streaming kernels once the batch fills the chip (documents of <= 8 rows: fused.hip's max-sim form, four candidates of a job
// per wave; 9 .. 16 rows: tile16.hip, two), else -- small batches, longer documents -- the one-workgroup-per-pair kernels.
ScorePlan plan_l2max_batch(const aspire_repset* q, const aspire_repset* c, int64_t max_job, bool one_form) {
    ScorePlan p{};
    const int64_t J = q->n, C = c->n;
    const int max_rows = p.max_rows = max_rows_of(q, c);
    const int64_t groups_bound = J * ((max_job + 3) / 4);
    const int form_t = tuning().ot_form;
    const bool big = hybrid_size_ok(groups_bound, C) && form_t != 1;
    // (small batches too: a wave walks an item's twelve stages in ~15 us, what a one-workgroup-per-pair launch takes anyway)
    // short queries against abstracts of up to 32 rows (config 4's shape): the CHUNK items of plan_ot_batch, max epilogue
    // (no solve runs, so none of otAspire's scaling / FUSED_* exclusions apply)
    if (q->max_len <= 8 && max_rows > 8 && max_rows <= kTileMaxRows && chunk_size_ok(C) && !one_form) {
        p.form = Form::Chunk;
        return p;
    }
    // whole abstracts of up to 32 rows against queries of 9 .. 16: the 16-row streaming kernel on record items, max epilogue (a
    // query of more than 16 rows would need its two halves' maxima joined across items: the per-candidate kernel keeps those)
    if (q->max_len <= 16 && max_rows > 16 && max_rows <= kTileMaxRows && chunk_size_ok(C) && !one_form) {
        p.form = Form::Rec16;
        return p;
    }
    // batches of <= 64 jobs of short documents: the streaming kernel's waves derive the tables themselves (fused.hip, SELF) --
    // one launch in front of the rank, at any size (2 x 20: 19 us either way)
    const bool self = form_t != 1 && max_rows <= 8 && J <= kSelfMaxJobs && !tuning().fused_noself && !one_form;
    // REVIEW: unlike stream_short, every OT_FORM pin from 2 up (tile, chunk, one) streams here, not `fused` alone.  Kept as it is.
    const bool streaming = form_t != 1 && (self || big || form_t >= 2 || groups_bound >= kL2StreamMinGroups) && !one_form;
    p.tables_first = !self;
    if (streaming && max_rows <= 8) p.form = self ? Form::FusedSelf : Form::FusedTables;
    // mostly short documents with a few of 9 .. 16 rows: the hybrid of plan_ot_batch (ScoreArgs::gate)
    else if (streaming && max_rows <= 16) p.form = big && form_t == 0 ? Form::Hybrid : Form::Stream16;
    // one workgroup per candidate against its job's query (small batches, documents of 17 .. 32 rows)
    else if (max_rows <= kTileMaxRows && !one_form) p.form = Form::Tiles;
    else p.form = Form::Generic;
    return p;
}

// ---- stage 1: the cost kernel of a chunk of workspace slots ---------------------------------------------------------------------
CostChoice cost_kernel_form(int T, const aspire_repset* q, const aspire_repset* c, int pairing, bool gram, bool tile_form,
                            bool tables_built, int64_t chunk_cands, int64_t jobs, int64_t max_job_groups, int64_t n_slots) {
    // many queries or long documents: Gram tiles on the matrix cores (gram.hip)
    if (gram) return {CostKernel::Gram, n_slots};
    const bool mapped = pairing == kPairMapped, cross = pairing == ASPIRE_PAIR_CROSS;
    const int form_t = tuning().ot_form;
    if (T == 1 && csr(q, c)) {
        // groups of four candidates x queries (MAPPED: an upper bound; the kernel reads the exact range from grp_off)
        const int64_t groups4 = mapped ? jobs * max_job_groups : (chunk_cands + 3) / 4 * (cross ? q->n : 0);
        // enough groups of 4 candidates to fill the chip: tiled form (lanes own finished (i,j) sums), one group per wave.
        // Small grids are latency bound: three waves per pair (a third of the coordinates each), persistent and software
        // pipelined (measured 15.6 us per launch at 50-250 pairs against 20-23 us for the tiled form with its stages split
        // over three or four waves).
        const bool tile = mapped ? tile_form : (cross && (form_t == 2 || (form_t != 1 && chip_filling(groups4))));
        return tile ? CostChoice{CostKernel::Tile, groups4} : CostChoice{CostKernel::Cost1, n_slots};
    }
    // documents of 9 .. 16 rows, enough pairs of candidates to fill the chip: the streaming kernel (tile16.hip)
    const int64_t items16 = mapped ? 2 * jobs * max_job_groups : (chunk_cands + 1) / 2 * q->n;
    if (T == 2 && tile16_path_ok(q, c, pairing) && (!mapped || tables_built) && form_t != 1 && (form_t == 2 || chip_filling(items16)))
        return {CostKernel::Tile16, items16};
    // CSR documents of more than 8 rows: every 8 x 8 sub-tile of every pair is an item of the small-pool kernel while the pairs
    // alone would not fill the chip
    if (csr(q, c) && n_slots < kSubTileMaxPairs) return {CostKernel::Cost1Sub, n_slots * T * T};
    return {CostKernel::Cost, n_slots};
}

// ---- stage 2: the solver of a launch of workspace slots -------------------------------------------------------------------------
SolveChoice solver_form(int T, int64_t n_slots, int max_rows, bool pair_outputs, int form_hint) {
    const int pinned = tuning().sinkhorn_form;
    const int form = pinned ? pinned : form_hint ? form_hint
                     : T == 1 ? (n_slots < kBlock16MinSlots ? 1 : n_slots < kBlockMinSlots ? 5 : 3)
                              : (n_slots >= kBlockMinSlotsLong ? 3 : 1);
    if (form < 3 || pair_outputs) return {Solver::Wave, 0, 0, false};      // (the block kernels write no pair outputs)
    // lanes per pair side and entries per lane side: the smallest block grid that covers max_rows
    const int r4 = (max_rows + 3) / 4;
    const bool dense = form == 6 || (form != 7 && n_slots >= (T == 1 ? kDenseMinSlots : kDenseMinSlotsLong));
    const bool repair = form != 4;      // pairs whose sums left fp32 range (NaN score) are solved again with the max-shifted solver
    if (T == 1) return form == 5 ? SolveChoice{Solver::Block, 4, 2, repair} : dense ? SolveChoice{Solver::Block, 1, 8, repair}
                                                                                    : SolveChoice{Solver::Block, 2, 4, repair};
    if (dense && r4 == 3) return {Solver::Block, 2, 6, repair};
    if (dense && r4 == 4) return {Solver::Block, 2, 8, repair};
    return {Solver::Block, 4, r4 < 3 ? 8 : r4 > 8 ? 8 : r4, repair};
}

}  // namespace aspire
