// The scoring entry points.  No kernel is defined here and no rule that picks one: every entry point reads argument checks, the
// plan of its family (forms.h: one pure decision function per family, every rule and threshold in forms.hip), a `switch` over the
// plan that carries it out through the launchers of the units that define the kernels (score_types.h lists them by unit:
// cost_valu.hip, sinkhorn.hip, batch_prep.hip, gram.hip, gramp.hip, generic.hip, fused.hip, tile16.hip), and the rank (topk.hip).
// Reference call structure:
//   src/learning/facetid_models/pair_distances.py:21-92, :138-186; src/evaluation/evaluate.py:58-76 (allenai/aspire).
//
// Top to bottom: argument checks and ScoreArgs fills (check_repsets, check_backward_sets, fill_set_args, fill_ot_args); the max-sim
// entry points and the backward of their aggregations (aspire_l2agg_backward_f32: checks here, the kernel in l2agg_bwd.hip), the checks of
// aspire_jointsm_backward_f32 (jointsm_bwd.hip), of the supervised-alignment pair aspire_l2sup_scores_f32 / _backward_f32 (l2sup.hip) and
// of the padded blocks' distance matrix aspire_sent_cdist_f32 / _backward_f32 (cdist_pair.hip); the workspace layouts of the batched
// / CHUNK / REC forms (batch_layout, l2_batch_layout, batch_tables) and launch_fused_form; otAspire per call (ot_run_tiles, ot_run)
// and its backward (aspire_ot_backward_f32: checks here, the kernel in ot_bwd.hip); the batched entry points (ot_rank_batch,
// aspire_l2max_rank_batch_f32), which share their argument checks and their rank with dotmax.hip through batch_host.h
// (batch_preamble, BatchRank); aspire_debug_score_form, which names the plan of a call without running it.
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <type_traits>

#include "common.h"
#include "forms.h"
#include "score_types.h"
#include "score_device.h"
#include "topk_device.h"
#include "batch_host.h"

namespace aspire {
namespace {

int check_repsets(const aspire_repset* q, const aspire_repset* c, int64_t D, int pairing) {
    ASPIRE_REQUIRE(q && c, ASPIRE_ERR_INVALID_ARG, "null repset");
    ASPIRE_REQUIRE(D == kD, ASPIRE_ERR_UNSUPPORTED, "encoding dim %lld unsupported (kernels are built for 768)",
                   (long long)D);
    ASPIRE_REQUIRE(pairing == ASPIRE_PAIR_CROSS || pairing == ASPIRE_PAIR_PAIRED, ASPIRE_ERR_INVALID_ARG,
                   "bad pairing %d", pairing);
    ASPIRE_REQUIRE(q->n >= 0 && c->n >= 0, ASPIRE_ERR_INVALID_ARG, "negative document count");
    // pair_distances.py:46  assert (qef_batch_size == cef_batch_size)
    ASPIRE_REQUIRE(pairing != ASPIRE_PAIR_PAIRED || q->n == c->n, ASPIRE_ERR_INVALID_ARG,
                   "paired scoring needs equal batch sizes (query %lld vs cand %lld)", (long long)q->n, (long long)c->n);
    ASPIRE_REQUIRE(q->ext >= 0 && c->ext >= 0, ASPIRE_ERR_INVALID_ARG, "negative ext");
    return ASPIRE_OK;
}

RepSet to_dev(const aspire_repset* s) { return RepSet{s->rows, s->start, s->len, s->n, s->ext}; }
// the rep sets of a call and what travels with them (a field added here reaches every entry point)
void fill_set_args(ScoreArgs& a, const aspire_repset* q, const aspire_repset* c, int pairing) {
    a.q = to_dev(q);
    a.c = to_dev(c);
    a.q_planes = q->planes;
    a.c_planes = c->planes;
    a.c_box = c->doc_box;
    a.pairing = pairing;
}

// What the backward entries (l2agg, jointsm, l2sup, ot) check first, alike: the sets, PAIRED only.  Yields the host-known bounds of
// the documents' rows.  (An entry's own argument checks follow, then its null-pointer check once there is a pair to write for.)
int check_backward_sets(const aspire_repset* q, const aspire_repset* c, int64_t D, int pairing, int& rows_q, int& rows_c) {
    if (int rc = check_repsets(q, c, D, pairing)) return rc;
    ASPIRE_REQUIRE(pairing == ASPIRE_PAIR_PAIRED, ASPIRE_ERR_UNSUPPORTED,
                   "the backward is built for ASPIRE_PAIR_PAIRED: with ASPIRE_PAIR_CROSS a document's gradient is a sum over many pairs, "
                   "which needs an accumulation across pairs that is not built");
    rows_q = q->ext > 0 ? q->ext : q->max_len;
    rows_c = c->ext > 0 ? c->ext : c->max_len;
    return ASPIRE_OK;
}

// the flags or'ed into the max-sim entry points' cdist_mode, taken off it
struct CdistFlags {
    bool one_form, center;
};
CdistFlags take_cdist_flags(int& cdist_mode) {
    const CdistFlags f{(cdist_mode & ASPIRE_CDIST_ONE_FORM) != 0, (cdist_mode & ASPIRE_CDIST_CENTER) != 0};
    cdist_mode &= ~(ASPIRE_CDIST_ONE_FORM | ASPIRE_CDIST_CENTER);
    return f;
}

// Query chunking.  CROSS: grid.x = candidates, grid.y = query chunks; queries are split over grid.y only while
// the grid is too small to fill 256 CUs several times over (each block re-reads its candidate from L2 per
// query chunk).
int query_chunks(ScoreArgs& a) {
    if (a.pairing == ASPIRE_PAIR_PAIRED) {
        a.q_per_block = 1;
        return 1;
    }
    int64_t chunks = 1;
    const int64_t target_blocks = 256 * 8;
    while (a.c.n * chunks < target_blocks && chunks < a.q.n) chunks *= 2;
    int64_t qpb = (a.q.n + chunks - 1) / chunks;
    chunks = (a.q.n + qpb - 1) / qpb;
    a.q_per_block = (int)qpb;
    return (int)chunks;
}

}  // namespace
}  // namespace aspire

using namespace aspire;

extern "C" int aspire_max_sents(void) { return generic_max_rows(); }

extern "C" int aspire_l2agg_scores_f32(const aspire_repset* q, const aspire_repset* c, int64_t D, int pairing,
                                       int cdist_mode, int agg, double temp, float* scores, float* pair_sims,
                                       float* pair_softmax, void* stream) {
    if (int rc = check_repsets(q, c, D, pairing)) return rc;
    ASPIRE_REQUIRE(agg == ASPIRE_AGG_MAX || agg == ASPIRE_AGG_TOP2 || agg == ASPIRE_AGG_ATTENTION, ASPIRE_ERR_INVALID_ARG,
                   "bad aggregation %d", agg);
    ASPIRE_REQUIRE(agg != ASPIRE_AGG_ATTENTION || temp > 0, ASPIRE_ERR_INVALID_ARG, "attention temperature must be positive");
    ASPIRE_REQUIRE(!pair_softmax || agg == ASPIRE_AGG_ATTENTION, ASPIRE_ERR_INVALID_ARG,
                   "pair_softmax is an output of the attention aggregation only");
    if (q->n == 0 || c->n == 0) return ASPIRE_OK;   // nothing to score (an empty pool has no buffers either)
    ASPIRE_REQUIRE(scores, ASPIRE_ERR_INVALID_ARG, "scores is null");
    ASPIRE_REQUIRE((!pair_sims && !pair_softmax) || (q->ext > 0 && c->ext > 0), ASPIRE_ERR_INVALID_ARG,
                   "pair outputs need padded extents (ext > 0)");
    const CdistFlags flags = take_cdist_flags(cdist_mode);
    ASPIRE_REQUIRE(!flags.one_form || agg == ASPIRE_AGG_MAX, ASPIRE_ERR_UNSUPPORTED, "ASPIRE_CDIST_ONE_FORM is built for the max-sim score only");
    ScoreArgs a{};
    fill_set_args(a, q, c, pairing);
    a.cdist_mode = cdist_mode;
    a.agg = agg;
    a.temp = temp;
    a.scores = scores;
    a.out_pairsims = pair_sims;
    a.out_plan = pair_softmax;
    a.center = flags.center;
    hipStream_t s = (hipStream_t)stream;
    const int rows_q = q->ext > 0 ? q->ext : q->max_len, rows_c = c->ext > 0 ? c->ext : c->max_len;
    const ScorePlan plan = plan_l2agg(q, c, pairing, agg, pair_sims != nullptr, flags.one_form);
    switch (plan.form) {
    case Form::Generic: return launch_pair_generic(a, 1, 0, rows_q, rows_c, s);
    case Form::GramPlanes:
    case Form::Gram: return launch_pair_gram_l2max(a, q->max_len, c->max_len, s);
    case Form::Stream16:
    case Form::FusedStream:
        a.cand0 = 0;
        a.cand1 = c->n;
        return plan.form == Form::Stream16 ? launch_pair_tile16_l2max(a, (c->n + 1) / 2, s)
                                           : launch_pair_fused_l2max(a, (c->n + 3) / 4 * q->n, s);
    default: break;      // Form::Tiles
    }
    const int qchunks = query_chunks(a);
    if (int rc = launch_l2max_tiles(a, plan.max_rows, qchunks, s)) return rc;
    return plan.then_generic ? launch_pair_generic(a, 1, plan.max_rows, rows_q, rows_c, s) : (int)ASPIRE_OK;
}

extern "C" int aspire_l2max_scores_f32(const aspire_repset* q, const aspire_repset* c, int64_t D, int pairing,
                                       int cdist_mode, float* scores, float* pair_sims, void* stream) {
    return aspire_l2agg_scores_f32(q, c, D, pairing, cdist_mode, ASPIRE_AGG_MAX, 1.0, scores, pair_sims, nullptr, stream);
}

extern "C" int aspire_l2agg_backward_f32(const aspire_repset* q, const aspire_repset* c, int64_t D, int pairing, int agg, double temp,
                                         const float* grad_scores, float* grad_q_rows, float* grad_c_rows, void* stream) {
    int rows_q, rows_c;
    if (int rc = check_backward_sets(q, c, D, pairing, rows_q, rows_c)) return rc;
    ASPIRE_REQUIRE(agg == ASPIRE_AGG_MAX || agg == ASPIRE_AGG_TOP2 || agg == ASPIRE_AGG_ATTENTION, ASPIRE_ERR_INVALID_ARG,
                   "bad aggregation %d", agg);
    ASPIRE_REQUIRE(agg != ASPIRE_AGG_ATTENTION || temp > 0, ASPIRE_ERR_INVALID_ARG, "attention temperature must be positive");
    if (q->n == 0) return ASPIRE_OK;                // no pair, no row
    ASPIRE_REQUIRE(grad_scores && grad_q_rows && grad_c_rows, ASPIRE_ERR_INVALID_ARG, "grad_scores, grad_q_rows or grad_c_rows is null");
    return launch_l2agg_backward(to_dev(q), to_dev(c), agg, (float)temp, grad_scores, grad_q_rows, grad_c_rows, rows_q, rows_c,
                                 (hipStream_t)stream);
}

// Backward of the joint soft-max alignment score (the forward is in jointsm.hip; the kernel in jointsm_bwd.hip)
extern "C" int aspire_jointsm_backward_f32(const aspire_repset* q, const aspire_repset* c, int64_t D, int pairing,
                                           const float* grad_scores, float* grad_q_rows, float* grad_c_rows, void* stream) {
    int rows_q, rows_c;
    if (int rc = check_backward_sets(q, c, D, pairing, rows_q, rows_c)) return rc;
    if (q->n == 0) return ASPIRE_OK;                // no pair, no row
    ASPIRE_REQUIRE(grad_scores && grad_q_rows && grad_c_rows, ASPIRE_ERR_INVALID_ARG, "grad_scores, grad_q_rows or grad_c_rows is null");
    return launch_jointsm_backward(to_dev(q), to_dev(c), grad_scores, grad_q_rows, grad_c_rows, rows_q, rows_c, (hipStream_t)stream);
}

// The supervised-alignment distances and their backward (kernels in l2sup.hip): PAIRED only, no pairing argument
extern "C" int aspire_l2sup_scores_f32(const aspire_repset* q, const aspire_repset* c, int64_t D, const int32_t* align, int weighted,
                                       float* scores, void* stream) {
    if (int rc = check_repsets(q, c, D, ASPIRE_PAIR_PAIRED)) return rc;
    if (q->n == 0) return ASPIRE_OK;
    ASPIRE_REQUIRE(align && scores, ASPIRE_ERR_INVALID_ARG, "align or scores is null");
    const int rows_q = q->ext > 0 ? q->ext : q->max_len, rows_c = c->ext > 0 ? c->ext : c->max_len;
    return launch_l2sup_scores(to_dev(q), to_dev(c), align, weighted != 0, scores, rows_q, rows_c, (hipStream_t)stream);
}

extern "C" int aspire_l2sup_backward_f32(const aspire_repset* q, const aspire_repset* c, int64_t D, const int32_t* align, int weighted,
                                         const float* grad_scores, float* grad_q_rows, float* grad_c_rows, void* stream) {
    int rows_q, rows_c;
    if (int rc = check_backward_sets(q, c, D, ASPIRE_PAIR_PAIRED, rows_q, rows_c)) return rc;
    if (q->n == 0) return ASPIRE_OK;
    ASPIRE_REQUIRE(align && grad_scores && grad_q_rows && grad_c_rows, ASPIRE_ERR_INVALID_ARG,
                   "align, grad_scores, grad_q_rows or grad_c_rows is null");
    return launch_l2sup_backward(to_dev(q), to_dev(c), align, weighted != 0, grad_scores, grad_q_rows, grad_c_rows, rows_q, rows_c,
                                 (hipStream_t)stream);
}

// The cross-document distance matrix of the padded blocks and its backward (kernels in cdist_pair.hip): PAIRED only, padded sets only
extern "C" int aspire_sent_cdist_f32(const aspire_repset* q, const aspire_repset* c, int64_t D, float* dist, void* stream) {
    int rows_q, rows_c;
    if (int rc = check_backward_sets(q, c, D, ASPIRE_PAIR_PAIRED, rows_q, rows_c)) return rc;
    ASPIRE_REQUIRE(q->ext > 0 && c->ext > 0, ASPIRE_ERR_INVALID_ARG, "the distance matrix needs padded extents (ext > 0)");
    if (q->n == 0) return ASPIRE_OK;
    ASPIRE_REQUIRE(dist, ASPIRE_ERR_INVALID_ARG, "dist is null");
    return launch_sent_cdist(to_dev(q), to_dev(c), dist, rows_q, rows_c, (hipStream_t)stream);
}

extern "C" int aspire_sent_cdist_backward_f32(const aspire_repset* q, const aspire_repset* c, int64_t D, const float* grad_dist,
                                              float* grad_q_rows, float* grad_c_rows, void* stream) {
    int rows_q, rows_c;
    if (int rc = check_backward_sets(q, c, D, ASPIRE_PAIR_PAIRED, rows_q, rows_c)) return rc;
    ASPIRE_REQUIRE(q->ext > 0 && c->ext > 0, ASPIRE_ERR_INVALID_ARG, "the distance matrix needs padded extents (ext > 0)");
    if (q->n == 0) return ASPIRE_OK;
    ASPIRE_REQUIRE(grad_dist && grad_q_rows && grad_c_rows, ASPIRE_ERR_INVALID_ARG, "grad_dist, grad_q_rows or grad_c_rows is null");
    return launch_sent_cdist_backward(to_dev(q), to_dev(c), grad_dist, grad_q_rows, grad_c_rows, rows_q, rows_c, (hipStream_t)stream);
}

namespace {
// bytes of workspace per pair slot at tile size T
size_t slot_bytes(int max_rows) {
    const int T = (max_rows + 7) / 8;
    return (size_t)(2 * 64 * T * T + 1) * sizeof(float);
}
constexpr size_t kWsCap = (size_t)1 << 30;  // suggested workspace is capped at 1 GiB; larger jobs run in chunks
constexpr size_t kWsSlack = 48;             // alignment of the box tables behind the pair slots
size_t align16(size_t n) { return (n + 15) & ~(size_t)15; }
// workspace bytes one candidate of a chunk needs: its pair slots (+ its bounding box on the matrix-core path)
size_t per_cand_bytes(const aspire_repset* q, const aspire_repset* c, int pairing) {
    return slot_bytes(max_rows_of(q, c)) * (pairing == ASPIRE_PAIR_CROSS ? (size_t)q->n : 1) +
           (gram_path_wanted(q, c, pairing) ? gram_extra_bytes_per_cand() : 0);
}
// candidates per chunk of a per-call otAspire workspace of `workspace_bytes` (the queries' boxes sit at its tail)
int64_t ot_cand_per_chunk(const aspire_repset* q, size_t workspace_bytes, size_t per_cand) {
    return (int64_t)((((workspace_bytes - qbox_bytes(q)) & ~(size_t)15) - 32) / per_cand);
}
}  // namespace

// (a multiple of 16 bytes: the rank scratch of aspire_ot_rank_f32 -- 64-bit keys -- sits right behind it)
extern "C" size_t aspire_ot_workspace_bytes(const aspire_repset* q, const aspire_repset* c, int pairing) {
    if (!q || !c || q->n <= 0 || c->n <= 0) return 0;
    const size_t per_cand = per_cand_bytes(q, c, pairing);
    const size_t full = per_cand * (size_t)c->n;
    if (full <= kWsCap) return align16(full + qbox_bytes(q) + kWsSlack);
    return align16((per_cand > kWsCap ? per_cand : kWsCap / per_cand * per_cand) + qbox_bytes(q) + kWsSlack);
}

namespace {
// rank request of aspire_ot_rank_f32 (k == 0: scores only)
struct RankReq {
    int64_t k, idx_base;
    float* top_scores;
    int64_t* top_idx;
    uint64_t* keys;
    // the rank of Q x C scores; its scratch sits `scratch_off` bytes into the call's workspace
    int rank(const float* scores, int64_t Q, int64_t C, void* workspace, size_t scratch_off, void* stream) const {
        if (k <= 0) return ASPIRE_OK;
        const size_t need = aspire_topk_workspace_bytes(Q, C, k);
        return topk_run(scores, Q, C, k, idx_base, top_scores, top_idx, keys, need ? (char*)workspace + scratch_off : nullptr, need, stream);
    }
};

int check_ot_params(const aspire_ot_params* prm, int want) {
    ASPIRE_REQUIRE(prm, ASPIRE_ERR_INVALID_ARG, "null params");
    ASPIRE_REQUIRE(want == ASPIRE_OT_DISTANCE || want == ASPIRE_OT_PLAN_SIM || want == ASPIRE_OT_SIMILARITY, ASPIRE_ERR_INVALID_ARG,
                   "bad want %d", want);
    ASPIRE_REQUIRE(prm->blur > 0 && prm->scaling > 0 && prm->scaling < 1 && prm->sent_sm_temp > 0,
                   ASPIRE_ERR_INVALID_ARG, "need blur > 0, 0 < scaling < 1, temp > 0");
    return ASPIRE_OK;
}

void fill_ot_args(ScoreArgs& a, const aspire_repset* q, const aspire_repset* c, int pairing, const aspire_ot_params* prm,
                  const float* diameter, int64_t diam_group, int want, float* scores) {
    fill_set_args(a, q, c, pairing);
    a.cdist_mode = prm->cdist_mode;
    a.blur = prm->blur;
    a.scaling = prm->scaling;
    a.temp = prm->sent_sm_temp;
    a.log_blur = std::log(prm->blur);
    a.log_scaling = std::log(prm->scaling);
    a.log2_blur = (float)(a.log_blur * 1.4426950408889634);
    a.log2_scaling = (float)(a.log_scaling * 1.4426950408889634);
    a.diameter = diameter;
    a.diam_group = diameter ? diam_group : 1;
    a.n_groups = diameter ? (c->n + diam_group - 1) / diam_group : 0;
    a.want = want;
    a.scores = scores;
    a.center = (prm->flags & ASPIRE_OT_FLAG_CENTER) != 0;
}

// the pair slots of `n_slots` pairs at `base` (cost tiles, -cdist tiles, squared diameters)
template <int T>
PairWs<T> pair_ws_at(void* base, int64_t n_slots) {
    PairWs<T> ws;
    ws.cost = (float*)base;
    ws.neg = ws.cost + n_slots * PairWs<T>::kEntries;
    ws.diam2 = ws.neg + n_slots * PairWs<T>::kEntries;
    return ws;
}
}  // namespace

// ---------------------------------------------------------------------------------------------
// The batched / CHUNK / REC forms: workspace layouts (the preparation kernels and their launchers: batch_prep.hip)
// ---------------------------------------------------------------------------------------------
namespace aspire {
namespace {

// Workspace of a batched call (byte offsets): otAspire's pair slots, then the tables the preparation kernels write, the hybrid
// forms' gate word and the rank scratch.
struct BatchLayout {
    size_t slots, qbox, cand_job, grp_job, grp_off, grp_rec, gate, topk, total;
};
BatchLayout batch_layout(int64_t J, int64_t C, int max_rows, int64_t max_job, int64_t k) {
    BatchLayout L{};
    size_t o = 0;
    L.slots = o; o = align16(o + slot_bytes(max_rows) * (size_t)C);
    L.qbox = o; o = align16(o + (size_t)J * 2 * kD * sizeof(float));
    L.cand_job = o; o = align16(o + (size_t)C * sizeof(int32_t));
    L.grp_job = o; o = align16(o + (size_t)(C / 4 + J + 1) * sizeof(int32_t));
    L.grp_off = o; o = align16(o + (size_t)(J + 1 > 64 ? J + 1 : 64) * sizeof(int32_t));
    // (documents of more than 8 rows: room for the CHUNK form's items, up to one per candidate)
    const size_t n_rec = max_rows > 16 ? 2 * (size_t)chunk_items_bound(J, C, max_job) + 1       // (16-row items, per query half)
                         : max_rows > 8 ? (size_t)chunk_items_bound(J, C, max_job) + 1 : (size_t)(C / 4 + J + 1);
    L.grp_rec = o; o = align16(o + n_rec * 16 * sizeof(int32_t));
    L.gate = o; o = align16(o + 16);
    L.topk = o; o = align16(o + aspire_topk_workspace_bytes(J, max_job, k));
    L.total = o;
    return L;
}
// tsAspire over batched jobs: no pair slots (max-sim is one launch), its own order
BatchLayout l2_batch_layout(int64_t J, int64_t C, int64_t max_job, int64_t k) {
    BatchLayout L{};
    size_t o = 0;
    L.cand_job = o; o = align16(o + (size_t)C * sizeof(int32_t));
    L.grp_job = o; o = align16(o + (size_t)(C / 4 + J + 1) * sizeof(int32_t));
    L.grp_off = o; o = align16(o + (size_t)(J + 1 > 64 ? J + 1 : 64) * sizeof(int32_t));
    L.grp_rec = o; o = align16(o + (2 * (size_t)chunk_items_bound(J, C, max_job) + 1) * 16 * sizeof(int32_t));     // (room for the CHUNK / REC forms' items)
    L.qbox = o; o = align16(o + (size_t)J * 2 * kD * sizeof(float));      // (written by the tables kernel, unused by max-sim)
    L.gate = o; o = align16(o + 16);
    L.topk = o; o = align16(o + aspire_topk_workspace_bytes(J, max_job, k));
    L.total = o;
    return L;
}
// the layout's pieces as pointers into a call's workspace (score_types.h: BatchTables)
BatchTables batch_tables(void* workspace, const BatchLayout& L) {
    char* w = (char*)workspace;
    return BatchTables{(float*)(w + L.slots), (float*)(w + L.qbox), (int32_t*)(w + L.cand_job), (int32_t*)(w + L.grp_job),
                       (int32_t*)(w + L.grp_off), (int32_t*)(w + L.grp_rec), (int32_t*)(w + L.gate), w + L.topk};
}
// MAPPED pairing (ScoreArgs::qmap): J jobs over C candidates in one launch, on the tables `t`
void fill_mapped_args(ScoreArgs& a, const BatchTables& t, const int32_t* job_off, int64_t J, int64_t C, int64_t max_job) {
    a.cand0 = 0;
    a.cand1 = C;
    a.qmap = t.cand_job;
    a.job_off = job_off;
    a.grp_off = t.grp_off;
    a.grp_job = t.grp_job;
    a.grp_rec = t.grp_rec;
    a.job0 = 0;
    a.job1 = (int32_t)J;
    a.max_job_groups = (int32_t)((max_job + 3) / 4);
}

// The fused launch of a call of short documents.  own_box: the kernel forms the query boxes itself (single-pool: ONE query;
// batched: the SELF form) and takes no qbox.  whole_call: every stage is wanted (always, but for the batched debug stage masks).
int launch_fused_form(const ScoreArgs& a, int64_t groups, bool own_box, bool whole_call, const float* qbox, const aspire_ot_params* prm,
                      hipStream_t s) {
#ifdef ASPIRE_EXPERIMENT_SPLIT      // round 5's role-split kernel: an experiment that lost, built only by tools/experiments/split/build.sh
    if (own_box && whole_call && split_path_ok(groups, prm) && a.c.n < ((int64_t)1 << 31) - 8) return launch_pair_split(a, s);
#endif
    return launch_pair_fused(a, groups, own_box ? nullptr : qbox, s);
}
}  // namespace
}  // namespace aspire

// ---------------------------------------------------------------------------------------------
// otAspire, one call = queries x one pool (CROSS) or pair by pair (PAIRED)
// ---------------------------------------------------------------------------------------------
namespace {

// The forms of documents of up to 32 rows of a call that ot_run has checked and described in `a` (a copy: what the forms set in it
// stays theirs).  q / c carry the row bound the kernels are to use (ot_run clamps max_len for pools with longer documents).
int ot_run_tiles(ScoreArgs a, const ScorePlan& plan, const aspire_repset* q, const aspire_repset* c, const aspire_ot_params* prm,
                 void* workspace, size_t workspace_bytes, hipStream_t stream, bool cost_only) {
    const int pairing = a.pairing;
    const bool extra = a.out_qdistr || a.out_cdistr || a.out_pairsims || a.out_plan;
    const size_t per_cand = per_cand_bytes(q, c, pairing);
    ASPIRE_REQUIRE(workspace && workspace_bytes >= per_cand + qbox_bytes(q) + kWsSlack, ASPIRE_ERR_INVALID_ARG,
                   "workspace too small: %zu bytes given, at least %zu needed (aspire_ot_workspace_bytes suggests %zu)",
                   workspace_bytes, per_cand, aspire_ot_workspace_bytes(q, c, pairing));
    a.cost_from_neg = plan.cost_from_neg;
    // query boxes sit at a fixed place (the tail of the workspace) so that every candidate chunk finds them
    float* qbox = (float*)((char*)workspace + ((workspace_bytes - qbox_bytes(q)) & ~(size_t)15));
    const int qchunks = query_chunks(a);
    a.cand0 = 0;
    a.cand1 = c->n;
    switch (plan.form) {
    case Form::FusedInbox:
    case Form::FusedQbox:      // costs and solves in ONE launch, no workspace slots, no candidate chunks (fused.hip)
        if (plan.qbox_first)
            if (int rc = launch_doc_box(a.q, qbox, stream)) return rc;
        return launch_fused_form(a, (c->n + 3) / 4 * q->n, plan.form == Form::FusedInbox, true, qbox, prm, stream);
    case Form::Chunk: {
        // counter and records at the front of the workspace; no candidate -> job table (ONE query)
        const BatchTables t{nullptr, qbox, nullptr, nullptr, (int32_t*)workspace, (int32_t*)((char*)workspace + 256), nullptr, nullptr};
        a.grp_off = t.grp_off;
        a.grp_rec = t.grp_rec;
        if (int rc = launch_chunk_prep(a, t, nullptr, 1, c->n, stream)) return rc;
        return launch_pair_fused_chunk(a, chunk_items_bound(1, c->n, c->n), qbox, stream);
    }
    default: break;      // Form::Tiles: the cost stage and the solve stage on workspace slots, in chunks of candidates
    }
    const int64_t cand_per_chunk = ot_cand_per_chunk(q, workspace_bytes, per_cand);
    const int64_t pairs_per_cand = pairing == ASPIRE_PAIR_PAIRED ? 1 : q->n;
    return dispatch_T(plan.max_rows, [&](auto tc) -> int {
        constexpr int T = decltype(tc)::value;
        for (int64_t c0 = 0; c0 < c->n; c0 += cand_per_chunk) {
            a.cand0 = c0;
            a.cand1 = c0 + cand_per_chunk < c->n ? c0 + cand_per_chunk : c->n;
            const int64_t n_slots = (a.cand1 - a.cand0) * pairs_per_cand;
            if (ot_chunk_one_wave(plan, q, c, pairing, a.cand1 - a.cand0, cost_only)) {
                if (int rc = launch_pair_one(a, n_slots, stream)) return rc;
                continue;
            }
            const PairWs<T> ws = pair_ws_at<T>(workspace, n_slots);
            float* cbox = (float*)(((uintptr_t)(ws.diam2 + n_slots) + 15) & ~(uintptr_t)15);
            if (int rc = launch_cost_stage(a, T, q, c, ws.cost, ws.neg, ws.diam2, n_slots, qchunks, plan.gram, qbox, cbox, c0 == 0, stream)) return rc;
            if (cost_only) continue;
            if (int rc = launch_sinkhorn_stage(a, T, ws.cost, ws.neg, ws.diam2, n_slots, plan.max_rows, extra, 0, stream)) return rc;
        }
        return (int)ASPIRE_OK;
    });
}

// One otAspire call: the argument checks, the plan (forms.hip: plan_ot), its launches, the rank.
int ot_run(const aspire_repset* q, const aspire_repset* c, int64_t D, int pairing, const aspire_ot_params* prm,
           const float* diameter, int64_t diam_group, int want, float* scores, float* out_qdistr, float* out_cdistr,
           float* out_pairsims, float* out_plan, void* workspace, size_t workspace_bytes, void* stream, const RankReq& rank,
           bool cost_only = false) {
    if (int rc = check_repsets(q, c, D, pairing)) return rc;
    if (q->n == 0 || c->n == 0) return ASPIRE_OK;   // nothing to score (an empty pool has no buffers either)
    if (int rc = check_ot_params(prm, want)) return rc;
    ASPIRE_REQUIRE(scores, ASPIRE_ERR_INVALID_ARG, "null scores");
    const bool extra = out_qdistr || out_cdistr || out_pairsims || out_plan;
    ASPIRE_REQUIRE(!extra || (q->ext > 0 && c->ext > 0), ASPIRE_ERR_INVALID_ARG, "pair outputs need padded extents (ext > 0)");
    ASPIRE_REQUIRE(!diameter || diam_group > 0, ASPIRE_ERR_INVALID_ARG, "diam_group must be positive");
    ScoreArgs a{};
    fill_ot_args(a, q, c, pairing, prm, diameter, diam_group, want, scores);
    a.out_qdistr = out_qdistr;
    a.out_cdistr = out_cdistr;
    a.out_pairsims = out_pairsims;
    a.out_plan = out_plan;
    hipStream_t s = (hipStream_t)stream;
    const ScorePlan plan = plan_ot(q, c, pairing, prm, OtAsked{extra, diameter != nullptr, cost_only, workspace != nullptr, workspace_bytes});
    const int rows_q = q->ext > 0 ? q->ext : q->max_len, rows_c = c->ext > 0 ? c->ext : c->max_len;
    if (plan.form == Form::Generic) {
        if (int rc = launch_pair_generic(a, 0, 0, rows_q, rows_c, s)) return rc;
    } else if (plan.form != Form::None) {
        // (CSR pools with longer documents: the tile kernels see the bound the plan clamped)
        const bool csr = q->ext == 0 && c->ext == 0;
        const aspire_repset q32 = csr ? tile_bound_set(q) : *q, c32 = csr ? tile_bound_set(c) : *c;
        if (int rc = ot_run_tiles(a, plan, &q32, &c32, prm, workspace, workspace_bytes, s, cost_only)) return rc;
        if (plan.then_generic)      // ... and the long-document kernel rewrites exactly those pairs
            if (int rc = launch_pair_generic(a, 0, kTileMaxRows, rows_q, rows_c, s)) return rc;
    }
    // the rank kernels follow the scores on the same stream (their scratch sits behind the OT workspace proper,
    // which aspire_ot_workspace_bytes keeps a multiple of 16 bytes)
    return rank.rank(scores, q->n, c->n, workspace, workspace_bytes, stream);
}
}  // namespace

extern "C" int aspire_ot_sinkhorn_f32(const aspire_repset* q, const aspire_repset* c, int64_t D, int pairing,
                                      const aspire_ot_params* prm, const float* diameter, int64_t diam_group, int want,
                                      float* scores, float* out_qdistr, float* out_cdistr, float* out_pairsims,
                                      float* out_plan, void* workspace, size_t workspace_bytes, void* stream) {
    return ot_run(q, c, D, pairing, prm, diameter, diam_group, want, scores, out_qdistr, out_cdistr, out_pairsims, out_plan,
                  workspace, workspace_bytes, stream, RankReq{0, 0, nullptr, nullptr, nullptr});
}

extern "C" int aspire_ot_backward_f32(const aspire_repset* q, const aspire_repset* c, int64_t D, int pairing, const aspire_ot_params* prm,
                                      const float* diameter, int64_t diam_group, int want, const float* grad_scores, float* grad_q,
                                      float* grad_c, void* stream) {
    int rows_q, rows_c;
    if (int rc = check_backward_sets(q, c, D, pairing, rows_q, rows_c)) return rc;
    if (int rc = check_ot_params(prm, want)) return rc;
    ASPIRE_REQUIRE(want != ASPIRE_OT_PLAN_SIM, ASPIRE_ERR_UNSUPPORTED,
                   "ASPIRE_OT_PLAN_SIM has no backward (the reference uses return_pair_sims at test time only)");
    ASPIRE_REQUIRE(!diameter || diam_group > 0, ASPIRE_ERR_INVALID_ARG, "diam_group must be positive");
    if (q->n == 0) return ASPIRE_OK;                // no pair, no row
    ASPIRE_REQUIRE(grad_scores && grad_q && grad_c, ASPIRE_ERR_INVALID_ARG, "grad_scores, grad_q or grad_c is null");
    return launch_ot_backward(to_dev(q), to_dev(c), prm, diameter, diam_group, want, grad_scores, grad_q, grad_c, rows_q, rows_c,
                              (hipStream_t)stream);
}

// Diagnostics: the cost stage of aspire_ot_sinkhorn_f32 alone (bench.py times the HBM-bound kernel of a pass this way).
extern "C" int aspire_debug_ot_cost_stage_f32(const aspire_repset* q, const aspire_repset* c, int64_t D, int pairing,
                                              const aspire_ot_params* prm, float* scores, void* workspace,
                                              size_t workspace_bytes, void* stream) {
    return ot_run(q, c, D, pairing, prm, nullptr, 0, ASPIRE_OT_DISTANCE, scores, nullptr, nullptr, nullptr, nullptr, workspace,
                  workspace_bytes, stream, RankReq{0, 0, nullptr, nullptr, nullptr}, true);
}

extern "C" size_t aspire_ot_rank_workspace_bytes(const aspire_repset* q, const aspire_repset* c, int64_t k) {
    if (!q || !c || q->n <= 0 || c->n <= 0) return 0;
    return aspire_ot_workspace_bytes(q, c, ASPIRE_PAIR_CROSS) + aspire_topk_workspace_bytes(q->n, c->n, k);
}

extern "C" int aspire_ot_rank_f32(const aspire_repset* q, const aspire_repset* c, int64_t D, const aspire_ot_params* prm,
                                  const float* diameter, int64_t diam_group, int want, float* scores, int64_t k,
                                  int64_t idx_base, float* top_scores, int64_t* top_idx, uint64_t* keys, void* workspace,
                                  size_t workspace_bytes, void* stream) {
    ASPIRE_REQUIRE(k > 0, ASPIRE_ERR_INVALID_ARG, "k must be positive");
    ASPIRE_REQUIRE((top_scores && top_idx) || keys, ASPIRE_ERR_INVALID_ARG, "need (top_scores, top_idx) or keys");
    ASPIRE_REQUIRE(q && c, ASPIRE_ERR_INVALID_ARG, "null repset");
    const size_t tneed = aspire_topk_workspace_bytes(q->n, c->n, k);
    ASPIRE_REQUIRE(workspace_bytes >= tneed, ASPIRE_ERR_INVALID_ARG, "workspace too small for the rank scratch");
    // the OT part is what is left, rounded down to 16 bytes so that the 64-bit rank scratch behind it stays aligned
    return ot_run(q, c, D, ASPIRE_PAIR_CROSS, prm, diameter, diam_group, want, scores, nullptr, nullptr, nullptr, nullptr, workspace,
                  (workspace_bytes - tneed) & ~(size_t)15, stream, RankReq{k, idx_base, top_scores, top_idx, keys});
}

// ---------------------------------------------------------------------------------------------
// Batched jobs: J independent (query, pool) re-ranks in one call.  Every entry point reads: its own set check, the shared
// argument checks (batch_host.h: batch_preamble), its workspace layout, its choice of form, its launches, the shared rank
// (BatchRank::rank).
// ---------------------------------------------------------------------------------------------
extern "C" size_t aspire_ot_rank_batch_workspace_bytes(const aspire_repset* q, const aspire_repset* c, int64_t max_job, int64_t k) {
    if (!q || !c || q->n <= 0 || c->n <= 0) return 0;
    const int mr = max_rows_of(q, c);
    return batch_layout(q->n, c->n, mr < 8 * kMaxT ? mr : 8 * kMaxT, max_job, k).total;
}

namespace {
int ot_rank_batch(const aspire_repset* q, const aspire_repset* c, int64_t D, const int32_t* job_off, int64_t max_job,
                  const aspire_ot_params* prm, int want, float* scores, int64_t k, const int32_t* job_base, float* top_scores,
                  int64_t* top_idx, uint64_t* keys, void* workspace, size_t workspace_bytes, void* stream, int stages) {
    if (int rc = check_repsets(q, c, D, ASPIRE_PAIR_CROSS)) return rc;
    if (int rc = check_ot_params(prm, want)) return rc;
    const int64_t J = q->n, C = c->n;
    BatchRank rank{J, max_job, k, top_scores, top_idx, keys, job_off, job_base, stream};
    bool go_on;
    if (int rc = batch_preamble(q, c, scores, rank, go_on); !go_on) return rc;
    hipStream_t s0 = (hipStream_t)stream;
    const int max_rows_all = max_rows_of(q, c);
    ASPIRE_REQUIRE(max_rows_all <= generic_max_rows(), ASPIRE_ERR_UNSUPPORTED,
                   "documents with more than %d sentence rows are not supported (got %d)", generic_max_rows(), max_rows_all);
    const BatchLayout L = batch_layout(J, C, max_rows_all < kTileMaxRows ? max_rows_all : kTileMaxRows, max_job, k);
    if (int rc = place_scratch(rank, workspace, workspace_bytes, L.total, L.topk, "aspire_ot_rank_batch_workspace_bytes")) return rc;
    const BatchTables t = batch_tables(workspace, L);
    if (!(stages & kStageRank)) rank.k = 0;      // (a stage mask of the debug entry point without the rank: scores only)
    ScoreArgs a{};
    fill_ot_args(a, q, c, kPairMapped, prm, nullptr, 0, want, scores);
    a.q_per_block = 1;
    fill_mapped_args(a, t, job_off, J, C, max_job);
    const int64_t groups_bound = J * ((max_job + 3) / 4);
    // Forms: forms.hip, plan_ot_batch.  (Chunks of jobs on two streams, Sinkhorn of chunk i beside the cost kernel of chunk i + 1,
    // were measured and dropped: 20 x 1000: 169 us on one stream, 213 / 266 / 403 us in 2 / 4 / 8 chunks -- cross-stream waits cost
    // more than they hide.)
    const ScorePlan plan = plan_ot_batch(q, c, max_job, prm, want, stages);
    const int max_rows = plan.max_rows;
    a.tile_form = plan.tile_form;
    if (plan.tables_first)
        if (int rc = launch_batch_tables(a, t, job_off, J, max_job, s0)) return rc;
    switch (plan.form) {
    case Form::None: break;
    case Form::Generic:      // (one workgroup per pair; the kernel finds a candidate's job by searching job_off)
        a.qmap = nullptr;
        if (int rc = launch_pair_generic(a, 0, 0, q->max_len, c->max_len, s0)) return rc;
        break;
    case Form::Chunk:
        if (int rc = launch_chunk_prep(a, t, job_off, J, max_job, s0)) return rc;
        if (int rc = launch_pair_fused_chunk(a, chunk_items_bound(J, C, max_job), t.qbox, s0)) return rc;
        break;
    case Form::Rec16: {
        if (int rc = launch_rec_prep(a, t, job_off, J, max_job, s0)) return rc;
        const int rc_run = dispatch_T(max_rows, [&](auto tc) -> int {
            constexpr int T = decltype(tc)::value;
            if constexpr (T >= 3) {
                const PairWs<T> ws = pair_ws_at<T>(t.slots, C);
                if (int rc = launch_pair_tile16_rec(a, T, ws.cost, ws.neg, ws.diam2, 2 * chunk_items_bound(J, C, max_job), t.qbox, s0)) return rc;
                return launch_sinkhorn_stage(a, T, ws.cost, ws.neg, ws.diam2, C, max_rows, false, 3, s0);
            }
            return (int)ASPIRE_ERR_UNSUPPORTED;
        });
        if (rc_run) return rc_run;
        break;
    }
    case Form::FusedSelf:
    case Form::FusedTables:
        if (int rc = launch_fused_form(a, groups_bound, plan.form == Form::FusedSelf, stages == kStageAll, t.qbox, prm, s0)) return rc;
        break;
    case Form::OneWave:
        if (int rc = launch_pair_one(a, C, s0)) return rc;
        break;
    case Form::Hybrid:
        if (int rc = arm_long_pair_gate(a, t.gate, C, s0)) return rc;
        if (int rc = launch_pair_fused(a, groups_bound, t.qbox, s0)) return rc;
        [[fallthrough]];      // ... in front of the 16-row cost kernel + the block solver
    default: {               // Form::Tiles
        const int rc_run = dispatch_T(max_rows, [&](auto tc) -> int {
            constexpr int T = decltype(tc)::value;
            const PairWs<T> ws = pair_ws_at<T>(t.slots, C);
            if (stages & kStageCost)
                if (int rc = launch_cost_stage(a, T, q, c, ws.cost, ws.neg, ws.diam2, C, 1, false, t.qbox, nullptr, true, s0)) return rc;
            if (stages & kStageSolve)
                if (int rc = launch_sinkhorn_stage(a, T, ws.cost, ws.neg, ws.diam2, C, max_rows, false, a.tile_form ? 3 : 0, s0)) return rc;
            return (int)ASPIRE_OK;
        });
        if (rc_run) return rc_run;
        if (plan.then_generic)      // documents beyond 32 rows: rewritten in front of the rank, as in ot_run
            if (int rc = launch_pair_generic(a, 0, max_rows, q->max_len, c->max_len, s0)) return rc;
    }
    }
    return rank.rank(scores);
}
}  // namespace

extern "C" int aspire_ot_rank_batch_f32(const aspire_repset* q, const aspire_repset* c, int64_t D, const int32_t* job_off,
                                        int64_t max_job, const aspire_ot_params* prm, int want, float* scores, int64_t k,
                                        const int32_t* job_base, float* top_scores, int64_t* top_idx, uint64_t* keys,
                                        void* workspace, size_t workspace_bytes, void* stream) {
    return ot_rank_batch(q, c, D, job_off, max_job, prm, want, scores, k, job_base, top_scores, top_idx, keys, workspace,
                         workspace_bytes, stream, kStageAll);
}

// ---- tsAspire over batched jobs ------------------------------------------------------------------------------------------
extern "C" size_t aspire_l2max_rank_batch_workspace_bytes(const aspire_repset* q, const aspire_repset* c, int64_t max_job, int64_t k) {
    if (!q || !c || q->n <= 0 || c->n <= 0) return 0;
    return l2_batch_layout(q->n, c->n, max_job, k).total;
}

extern "C" int aspire_l2max_rank_batch_f32(const aspire_repset* q, const aspire_repset* c, int64_t D, const int32_t* job_off,
                                           int64_t max_job, int cdist_mode, float* scores, int64_t k, const int32_t* job_base,
                                           float* top_scores, int64_t* top_idx, uint64_t* keys, void* workspace,
                                           size_t workspace_bytes, void* stream) {
    if (int rc = check_repsets(q, c, D, ASPIRE_PAIR_CROSS)) return rc;
    const int64_t J = q->n, C = c->n;
    BatchRank rank{J, max_job, k, top_scores, top_idx, keys, job_off, job_base, stream};
    bool go_on;
    if (int rc = batch_preamble(q, c, scores, rank, go_on); !go_on) return rc;
    hipStream_t s0 = (hipStream_t)stream;
    const int max_rows = max_rows_of(q, c);
    ASPIRE_REQUIRE(max_rows <= generic_max_rows(), ASPIRE_ERR_UNSUPPORTED, "documents with more than %d sentence rows are not supported (got %d)",
                   generic_max_rows(), max_rows);
    const BatchLayout L = l2_batch_layout(J, C, max_job, k);
    if (int rc = place_scratch(rank, workspace, workspace_bytes, L.total, L.topk, "aspire_l2max_rank_batch_workspace_bytes")) return rc;
    const BatchTables t = batch_tables(workspace, L);
    const CdistFlags flags = take_cdist_flags(cdist_mode);
    ScoreArgs a{};
    fill_set_args(a, q, c, kPairMapped);
    a.cdist_mode = cdist_mode;
    a.center = flags.center;
    a.agg = ASPIRE_AGG_MAX;
    a.temp = 1.0;
    a.scores = scores;
    fill_mapped_args(a, t, job_off, J, C, max_job);
    const int64_t groups_bound = J * ((max_job + 3) / 4);
    const ScorePlan plan = plan_l2max_batch(q, c, max_job, flags.one_form);      // forms.hip
    if (plan.tables_first)
        if (int rc = launch_batch_tables(a, t, job_off, J, max_job, s0)) return rc;
    int rc = ASPIRE_OK;
    switch (plan.form) {
    case Form::Chunk:
        if ((rc = launch_chunk_prep(a, t, job_off, J, max_job, s0))) return rc;
        rc = launch_pair_fused_chunk_l2max(a, chunk_items_bound(J, C, max_job), s0);
        break;
    case Form::Rec16:
        if ((rc = launch_rec_prep(a, t, job_off, J, max_job, s0))) return rc;
        rc = launch_pair_tile16_rec_l2max(a, 2 * chunk_items_bound(J, C, max_job), s0);
        break;
    case Form::FusedSelf:
    case Form::FusedTables: rc = launch_pair_fused_l2max(a, groups_bound, s0, plan.form == Form::FusedSelf); break;
    case Form::Hybrid:
        if ((rc = arm_long_pair_gate(a, t.gate, C, s0))) return rc;
        if ((rc = launch_pair_fused_l2max(a, groups_bound, s0))) return rc;
        [[fallthrough]];
    case Form::Stream16: rc = launch_pair_tile16_l2max(a, 2 * groups_bound, s0); break;
    case Form::Tiles: rc = launch_l2max_tiles(a, plan.max_rows, 1, s0); break;
    default: rc = launch_pair_generic(a, 1, 0, q->max_len, c->max_len, s0); break;      // Form::Generic
    }
    if (rc) return rc;
    return rank.rank(scores);
}

// Diagnostics: chosen stages of aspire_ot_rank_batch_f32 on the caller's stream alone (1 tables + query boxes, 2 cost
// kernel, 4 Sinkhorn kernel, 8 rank) -- bench.py times each stage of a pass this way, after a full call has filled the
// workspace.
extern "C" int aspire_debug_ot_rank_batch_stages_f32(const aspire_repset* q, const aspire_repset* c, int64_t D,
                                                     const int32_t* job_off, int64_t max_job, const aspire_ot_params* prm,
                                                     int want, float* scores, int64_t k, float* top_scores, int64_t* top_idx,
                                                     void* workspace, size_t workspace_bytes, void* stream, int stages) {
    ASPIRE_REQUIRE(stages > 0 && stages <= kStageAll, ASPIRE_ERR_INVALID_ARG, "bad stage mask %d", stages);
    return ot_rank_batch(q, c, D, job_off, max_job, prm, want, scores, k, nullptr, top_scores, top_idx, nullptr, workspace,
                         workspace_bytes, stream, stages);
}

extern "C" int aspire_group_diameter_f32(const aspire_repset* q, const aspire_repset* c, int64_t D, int pairing,
                                         int64_t group, float* diameter, void* stream) {
    if (int rc = check_repsets(q, c, D, pairing)) return rc;
    ASPIRE_REQUIRE(group > 0 && diameter, ASPIRE_ERR_INVALID_ARG, "group must be positive, diameter non-null");
    if (q->n == 0 || c->n == 0) return ASPIRE_OK;
    ScoreArgs a{};
    fill_set_args(a, q, c, pairing);
    const int64_t ngroups = (c->n + group - 1) / group;
    const int64_t blocks = pairing == ASPIRE_PAIR_PAIRED ? ngroups : ngroups * q->n;     // (query, group) folded into grid.x
    ASPIRE_REQUIRE(blocks < ((int64_t)1 << 31), ASPIRE_ERR_UNSUPPORTED, "too many (query, group) boxes: %lld", (long long)blocks);
    return launch_group_diameter(a, group, ngroups, blocks, diameter, (hipStream_t)stream);
}

// Diagnostics: the family a call would take, as short text -- the plan of the entry family `kind` and, where the plan runs the
// stages on workspace slots, their kernels for the call's first chunk.  Runs no kernel and needs no GPU; the only place that
// renders a plan as text.  Batched kinds take the jobs as equal shares of the candidates (max_job = ceil(c->n / q->n)).
extern "C" int aspire_debug_score_form(int kind, const aspire_repset* q, const aspire_repset* c, int pairing, const aspire_ot_params* prm,
                                       int asked, size_t workspace_bytes, char* buf, size_t len) {
    ASPIRE_REQUIRE(q && c && buf && len > 0, ASPIRE_ERR_INVALID_ARG, "null repset / buffer");
    ASPIRE_REQUIRE(q->n > 0 && c->n > 0, ASPIRE_ERR_INVALID_ARG, "an empty call has no form");
    const bool ot = kind == ASPIRE_FORM_OT || kind == ASPIRE_FORM_OT_BATCH;
    ASPIRE_REQUIRE(!ot || prm, ASPIRE_ERR_INVALID_ARG, "null params");
    const int stages = (asked >> 8) & kStageAll ? (asked >> 8) & kStageAll : kStageAll;
    const bool extra = asked & ASPIRE_ASKED_PAIR_OUTPUTS, cost_only = asked & ASPIRE_ASKED_COST_ONLY;
    const int64_t J = q->n, C = c->n, max_job = (C + J - 1) / J;
    static const char* const form_names[] = {"none", "generic", "gram-planes", "gram", "stream16", "fused-stream", "fused-inbox", "fused-qbox",
                                             "fused-self", "fused-tables", "chunk", "rec16", "one-wave", "tiles", "hybrid"};
    static const char* const cost_names[] = {"gram", "tile", "cost1", "tile16", "cost1-sub", "cost"};
    ScorePlan plan{};
    char stage_text[64] = "";
    auto render_stages = [&](const CostChoice* cost, const SolveChoice* solve) {
        size_t n = 0;
        if (cost) n += snprintf(stage_text + n, sizeof(stage_text) - n, " cost=%s", cost_names[(int)cost->kernel]);
        if (solve && solve->kernel == Solver::Wave) snprintf(stage_text + n, sizeof(stage_text) - n, " solve=wave");
        else if (solve) snprintf(stage_text + n, sizeof(stage_text) - n, " solve=block%dx%d%s", solve->lanes * solve->lanes, solve->per_lane,
                                 solve->repair ? "+repair" : "");
    };
    if (kind == ASPIRE_FORM_L2AGG) {
        plan = plan_l2agg(q, c, pairing, asked & ASPIRE_ASKED_AGG_OTHER ? ASPIRE_AGG_TOP2 : ASPIRE_AGG_MAX, extra, asked & ASPIRE_ASKED_ONE_FORM);
    } else if (kind == ASPIRE_FORM_L2MAX_BATCH) {
        plan = plan_l2max_batch(q, c, max_job, asked & ASPIRE_ASKED_ONE_FORM);
    } else if (kind == ASPIRE_FORM_OT) {
        const bool csr = q->ext == 0 && c->ext == 0;
        const aspire_repset q32 = csr ? tile_bound_set(q) : *q, c32 = csr ? tile_bound_set(c) : *c;
        if (!workspace_bytes) workspace_bytes = aspire_ot_workspace_bytes(&q32, &c32, pairing);
        plan = plan_ot(q, c, pairing, prm, OtAsked{extra, (asked & ASPIRE_ASKED_DIAMETERS) != 0, cost_only, true, workspace_bytes});
        if (plan.form == Form::Tiles) {
            const size_t per_cand = per_cand_bytes(&q32, &c32, pairing);
            ASPIRE_REQUIRE(workspace_bytes >= per_cand + qbox_bytes(q) + kWsSlack, ASPIRE_ERR_INVALID_ARG, "workspace too small");
            const int64_t per_chunk = ot_cand_per_chunk(q, workspace_bytes, per_cand), cands = per_chunk < C ? per_chunk : C;
            const int64_t n_slots = cands * (pairing == ASPIRE_PAIR_PAIRED ? 1 : J);
            const int T = (plan.max_rows + 7) / 8;
            if (ot_chunk_one_wave(plan, &q32, &c32, pairing, cands, cost_only)) {
                plan.form = Form::OneWave;
            } else {
                const CostChoice cost = cost_kernel_form(T, &q32, &c32, pairing, plan.gram, false, false, cands, 0, 0, n_slots);
                const SolveChoice solve = solver_form(T, n_slots, plan.max_rows, extra, 0);
                render_stages(&cost, cost_only ? nullptr : &solve);
            }
        }
    } else if (kind == ASPIRE_FORM_OT_BATCH) {
        plan = plan_ot_batch(q, c, max_job, prm, asked & ASPIRE_ASKED_PLAN_SIM ? ASPIRE_OT_PLAN_SIM : ASPIRE_OT_SIMILARITY, stages);
        const int T = (plan.max_rows + 7) / 8;
        const SolveChoice solve = solver_form(T, C, plan.max_rows, false, plan.tile_form || plan.form == Form::Rec16 ? 3 : 0);
        if (plan.form == Form::Rec16) {
            render_stages(nullptr, &solve);
        } else if (plan.form == Form::Tiles || plan.form == Form::Hybrid) {
            const CostChoice cost = cost_kernel_form(T, q, c, kPairMapped, false, plan.tile_form, true, C, J, (max_job + 3) / 4, C);
            render_stages(stages & kStageCost ? &cost : nullptr, stages & kStageSolve ? &solve : nullptr);
        }
    } else {
        ASPIRE_REQUIRE(false, ASPIRE_ERR_INVALID_ARG, "bad form kind %d", kind);
    }
    char text[128];
    const int n = snprintf(text, sizeof(text), "%s%s%s%s%s", plan.tables_first ? "tables+" : "", plan.qbox_first ? "qbox+" : "",
                           form_names[(int)plan.form], plan.then_generic ? "+generic" : "", stage_text);
    ASPIRE_REQUIRE((size_t)n + 1 <= len, ASPIRE_ERR_INVALID_ARG, "buffer too small");
    memcpy(buf, text, (size_t)n + 1);
    return ASPIRE_OK;
}
