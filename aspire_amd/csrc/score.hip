// Host dispatch of the scoring entry points: which kernel family scores a pair.  No kernel is defined here; every launch goes
// through the launcher of the unit that defines the kernel (score_types.h lists them by unit: cost_valu.hip, sinkhorn.hip,
// batch_prep.hip, gram.hip, gramp.hip, generic.hip, fused.hip, tile16.hip; the rank: topk.hip).  Reference call structure:
//   src/learning/facetid_models/pair_distances.py:21-92, :138-186; src/evaluation/evaluate.py:58-76 (allenai/aspire).
//
// Top to bottom: argument checks and ScoreArgs fills (check_repsets, check_backward_sets, fill_set_args, fill_ot_args); the max-sim
// entry points and the backward of their aggregations (aspire_l2agg_backward_f32: checks here, the kernel in l2agg_bwd.hip), the checks of
// aspire_jointsm_backward_f32 (jointsm_bwd.hip), of the supervised-alignment pair aspire_l2sup_scores_f32 / _backward_f32 (l2sup.hip) and
// of the padded blocks' distance matrix aspire_sent_cdist_f32 / _backward_f32 (cdist_pair.hip); the
// host helpers of the batched / CHUNK / REC forms -- form rules (chunk_size_ok, one_wave_form_ok, sinkhorn_form_honours_gate),
// workspace layouts (batch_layout, l2_batch_layout, batch_tables), launch_fused_form; otAspire per call (ot_run_tiles, ot_run)
// and its backward (aspire_ot_backward_f32: checks here, the kernel in ot_bwd.hip);
// the batched entry points (ot_rank_batch, aspire_l2max_rank_batch_f32).  Which kernel family scores a pair decides the pair's
// bits, so every rule that picks one is written once and asked by every entry point; the batched entry points share their
// argument checks and their rank with dotmax.hip through batch_host.h (batch_preamble, BatchRank).
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <type_traits>

#include "common.h"
#include "tuning.h"
#include "score_types.h"
#include "score_device.h"
#include "topk_device.h"
#include "batch_host.h"

namespace aspire {
namespace {

// Groups of four candidates from which the fused streaming kernel (fused.hip) is ahead of the small-pool kernels, documents of
// <= 8 rows (tools/otbatchcross.py: one query x one pool 750 groups 39 against 46 us, 2000 groups 59 / 94; batched jobs 500
// groups 33 / 37, 1600 groups 45 / 79).  Below, a call is latency bound and the small-pool kernels' shorter chains win.
constexpr int64_t kStreamMinGroups1 = 640, kStreamMinGroupsBatch = 512;

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

int max_rows_of(const aspire_repset* q, const aspire_repset* c) {
    const int mq = q->ext > 0 ? q->ext : q->max_len;
    const int mc = c->ext > 0 ? c->ext : c->max_len;
    return mq > mc ? mq : mc;
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
    const bool one_form = (cdist_mode & ASPIRE_CDIST_ONE_FORM) != 0, center = (cdist_mode & ASPIRE_CDIST_CENTER) != 0;
    cdist_mode &= ~(ASPIRE_CDIST_ONE_FORM | ASPIRE_CDIST_CENTER);
    ASPIRE_REQUIRE(!one_form || agg == ASPIRE_AGG_MAX, ASPIRE_ERR_UNSUPPORTED, "ASPIRE_CDIST_ONE_FORM is built for the max-sim score only");
    ScoreArgs a{};
    fill_set_args(a, q, c, pairing);
    a.cdist_mode = cdist_mode;
    a.agg = agg;
    a.temp = temp;
    a.scores = scores;
    a.out_pairsims = pair_sims;
    a.out_plan = pair_softmax;
    a.center = center;
    if (one_form)      // every pair through the long-form kernel, whatever the size of the call (include/aspire_hip.h)
        return launch_pair_generic(a, 1, 0, q->ext > 0 ? q->ext : q->max_len, c->ext > 0 ? c->ext : c->max_len, (hipStream_t)stream);
    // both sides carry fp16 planes: the matrix-pipe tiles (gramp.hip) whatever the number of queries
    if (agg == ASPIRE_AGG_MAX && !pair_sims && gram_planes_wanted_l2max(q, c, pairing))
        return launch_pair_gram_l2max(a, q->max_len, c->max_len, (hipStream_t)stream);
    // ONE query against a big pool of 9 .. 16-row documents: the streaming kernel's max-sim form (tile16.hip)
    if (agg == ASPIRE_AGG_MAX && !pair_sims && q->n == 1 && c->n >= 4096 && tile16_path_ok(q, c, pairing) &&
        pairing == ASPIRE_PAIR_CROSS && tuning().cost_path != 1 && tuning().ot_form != 1) {
        a.cand0 = 0;
        a.cand1 = c->n;
        return launch_pair_tile16_l2max(a, (c->n + 1) / 2, (hipStream_t)stream);
    }
    if (agg == ASPIRE_AGG_MAX && !pair_sims && gram_path_wanted(q, c, pairing))
        return launch_pair_gram_l2max(a, q->max_len, c->max_len, (hipStream_t)stream);
    // Few queries against a big pool of short documents (CSR): the fused kernel's streaming phase with a max epilogue --
    // four candidates per wave, dot products on the matrix pipe (l2max_kernel<1> is one workgroup per candidate with VALU
    // difference sums: 114 us at 1 x 20 000 against the stream's 88)
    {
        const int form_t = tuning().ot_form;
        const int64_t groups4 = (c->n + 3) / 4 * q->n;
        if (agg == ASPIRE_AGG_MAX && !pair_sims && pairing == ASPIRE_PAIR_CROSS && fused_path_ok(q, c) &&
            (form_t == 3 || (form_t == 0 && groups4 >= (q->n == 1 ? kStreamMinGroups1 : 2048)))) {
            a.cand0 = 0;
            a.cand1 = c->n;
            return launch_pair_fused_l2max(a, groups4, (hipStream_t)stream);
        }
    }
    // Documents beyond the tile kernels' 32 rows (max-sim only): padded tensors that wide go through the one-workgroup-
    // per-pair kernel for every pair; CSR pools run the tile kernel on 32-row tiles first (it covers every pair of short
    // documents) and the long-document kernel then rewrites the pairs that hold a longer one.
    const int rows_q = q->ext > 0 ? q->ext : q->max_len, rows_c = c->ext > 0 ? c->ext : c->max_len;
    const bool long_docs = max_rows_of(q, c) > 8 * kMaxT;
    if (long_docs && (q->ext > 0 || c->ext > 0)) return launch_pair_generic(a, 1, 0, rows_q, rows_c, (hipStream_t)stream);
    const int qchunks = query_chunks(a);
    const int tile_rows = long_docs ? 8 * kMaxT : max_rows_of(q, c);
    const int rc_tiles = launch_l2max_tiles(a, tile_rows, qchunks, (hipStream_t)stream);
    if (rc_tiles || !long_docs) return rc_tiles;
    return launch_pair_generic(a, 1, 8 * kMaxT, rows_q, rows_c, (hipStream_t)stream);
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
size_t qbox_bytes(const aspire_repset* q) { return (size_t)q->n * 2 * kD * sizeof(float); }
constexpr size_t kWsCap = (size_t)1 << 30;  // suggested workspace is capped at 1 GiB; larger jobs run in chunks
constexpr size_t kWsSlack = 48;             // alignment of the box tables behind the pair slots
size_t align16(size_t n) { return (n + 15) & ~(size_t)15; }
// workspace bytes one candidate of a chunk needs: its pair slots (+ its bounding box on the matrix-core path)
size_t per_cand_bytes(const aspire_repset* q, const aspire_repset* c, int pairing) {
    return slot_bytes(max_rows_of(q, c)) * (pairing == ASPIRE_PAIR_CROSS ? (size_t)q->n : 1) +
           (gram_path_wanted(q, c, pairing) ? gram_extra_bytes_per_cand() : 0);
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

// The hybrid forms (fused kernel in front of the 16-row kernels, ScoreArgs::gate) need a solve stage that leaves the short pairs'
// scores alone: the block kernels and their repair kernel check the gate, the one-solve-per-wave kernel (SINKHORN=wave) does not.
bool sinkhorn_form_honours_gate() {
    const int f = tuning().sinkhorn_form;
    return f == 0 || f == 3 || f == 5 || f == 6 || f == 7;
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
// The batched / CHUNK / REC forms: form rules and workspace layouts (the preparation kernels and their launchers: batch_prep.hip)
// ---------------------------------------------------------------------------------------------
namespace aspire {
namespace {

// smallest pool / batch (candidates) that takes the CHUNK / REC forms (below: the small-batch kernels; tools/csfbench.py sweeps)
constexpr int64_t kChunkMinCands = 256;
// the size rule of the CHUNK / REC forms: pinned (OT_FORM 4), or by default from kChunkMinCands candidates in the call
bool chunk_size_ok(int64_t C) {
    const int form_t = tuning().ot_form;
    return form_t == 4 || (form_t == 0 && C >= kChunkMinCands);
}
// pairs of short documents per call that take pair_one_kernel (tools/experiments/singlejob.py sweeps)
constexpr int64_t kOneMinPairs = 1, kOneMaxPairs = 8192;        // (ONE form for every small grid: a pair scored alone, in a subset or in a shard gets the same bits)
// May a call of `pairs` pairs of documents of <= 8 rows take the one-launch form (pair_one_kernel: one wave per pair, costs and
// solve)?  The single-pool and the batched entry points ask the same question, so that a pair gets the same kernel -- the same
// bits -- whether it is scored in a call of its own or in a batch.
//   plain_call: CSR sets, no Gram tiles, every stage of the call wanted.  Single-pool: ext == 0 on both sides && !gram &&
//               !cost_only; batched: the full stage mask (batched sets are CSR and never take the Gram tiles).
//   small_grid: the call stays below the throughput kernels.  The two callers' rules differ and stay their own: single-pool calls
//               go by groups of four (CROSS pairing from 2048 groups: the tiled cost kernel's grid), batches by !a.tile_form
//               (from kStreamMinGroupsBatch groups the fused kernel, which also carries the OT_FORM pins 2 and 3).
bool one_wave_form_ok(int64_t pairs, bool plain_call, bool small_grid) {
    const int form_t = tuning().ot_form;
    return plain_call && small_grid && pairs >= kOneMinPairs && pairs <= kOneMaxPairs &&
           (form_t == 5 || (form_t == 0 && tuning().sinkhorn_form == 0 && tuning().cost_path == 0 && tuning().cost1_blocks == 0));
}

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

// The tile-kernel forms (documents of up to 32 rows) of a call that ot_run has checked and described in `a`: non-empty sets, sound
// parameters, a.scores set.  q / c carry the row bound the kernels are to use (ot_run clamps max_len for pools with longer
// documents).  Scores only: the rank is ot_run's.
int ot_run_tiles(ScoreArgs a, const aspire_repset* q, const aspire_repset* c, const aspire_ot_params* prm, void* workspace,
                 size_t workspace_bytes, hipStream_t stream, bool cost_only) {
    const int pairing = a.pairing;
    const float* diameter = a.diameter;
    const bool extra = a.out_qdistr || a.out_cdistr || a.out_pairsims || a.out_plan;
    const int max_rows = max_rows_of(q, c);
    const size_t per_cand = per_cand_bytes(q, c, pairing);
    // ONE query against a big pool of 9 .. 16-row documents: the streaming kernel (tile16.hip) beats the 32-column Gram tiles,
    // whose 12 .. 16 real query rows fill a third to a half of the MFMA tile (1 x 20 000 x 12 otAspire: 247 vs 363 us; at two
    // queries they tie, from three the Gram tiles win: 623 vs 565 us)
    // both sides on fp16 planes, the pool's boxes cached: the plane tiles whatever the number of queries (gram.hip)
    const bool planes_ot = !extra && gram_planes_wanted_ot(q, c, pairing, diameter != nullptr) && tuning().ot_form == 0;
    const bool stream16 = !planes_ot && q->n == 1 && c->n >= 4096 && tile16_path_ok(q, c, pairing) && tuning().cost_path != 1 &&
                          tuning().ot_form != 1;
    const int form_t = tuning().ot_form;
    // ONE short query (facet-selected rows) against a pool of abstracts of up to 32 rows: the fused kernel's CHUNK form, as in
    // ot_rank_batch (1 x 20 000 x (3..20): 674 us on the Gram tiles + block Sinkhorn before) -- the item records and their counter
    // take the (unused) front of the pair-slot workspace.  (From kChunkMinCands candidates even where the form is pinned: the
    // call's workspace is sized for the pair slots.)
    const bool chunk1 = pairing == ASPIRE_PAIR_CROSS && q->n == 1 && q->ext == 0 && c->ext == 0 && q->max_len <= 8 && c->max_len > 8 &&
                        c->max_len <= 8 * kMaxT && c->n >= kChunkMinCands && c->n < ((int64_t)1 << 30) && !extra && !cost_only && !diameter &&
                        chunk_size_ok(c->n) && prm->scaling >= 0.25 && !tuning().fused_nosolve && !tuning().fused_valu &&
                        tuning().cost_path == 0 && workspace &&
                        (size_t)(chunk_items_bound(1, c->n, c->n) + 2) * 64 + 256 + qbox_bytes(q) + 64 <= workspace_bytes;
    const bool gram = (gram_path_wanted(q, c, pairing) || planes_ot) && !stream16 && !chunk1;
    ASPIRE_REQUIRE(workspace && workspace_bytes >= per_cand + qbox_bytes(q) + kWsSlack, ASPIRE_ERR_INVALID_ARG,
                   "workspace too small: %zu bytes given, at least %zu needed (aspire_ot_workspace_bytes suggests %zu)",
                   workspace_bytes, per_cand, aspire_ot_workspace_bytes(q, c, pairing));
    // the matrix-pipe cost tiles derive -cdist and geomloss's cost from ONE distance: they store -cdist only and the solve stage takes
    // cost = max(cdist, 1e-4) from it -- half the tile bytes written and read (the debug cost stage keeps both buffers)
    a.cost_from_neg = gram && !cost_only;
    const int qchunks = query_chunks(a);
    const int64_t cand_per_chunk = (int64_t)((((workspace_bytes - qbox_bytes(q)) & ~(size_t)15) - 32) / per_cand);
    const int64_t pairs_per_cand = pairing == ASPIRE_PAIR_PAIRED ? 1 : q->n;
    // query boxes sit at a fixed place (the tail of the workspace) so that every candidate chunk finds them
    float* qbox = (float*)((char*)workspace + ((workspace_bytes - qbox_bytes(q)) & ~(size_t)15));
    // Few queries against a big pool of short documents: costs and solves in ONE launch, no workspace slots, no candidate
    // chunks (fused.hip).
    const int64_t groups4_all = (c->n + 3) / 4 * q->n;
    const bool fused = pairing == ASPIRE_PAIR_CROSS && !extra && !gram && !cost_only && fused_path_ok(q, c) &&
                       (form_t == 3 || (form_t == 0 && groups4_all >= (q->n == 1 ? kStreamMinGroups1 : 2048)));
    if (fused) {
        a.cand0 = 0;
        a.cand1 = c->n;
        const bool inbox = fused_inbox_ok(q, diameter);      // ONE query: the kernel forms its box itself
        if (!diameter && !inbox)     // per-coordinate boxes of the queries (the kernel adds each candidate's rows)
            if (int rc = launch_doc_box(a.q, qbox, stream)) return rc;
        return launch_fused_form(a, groups4_all, inbox, true, qbox, prm, stream);
    }
    if (chunk1) {
        a.cand0 = 0;
        a.cand1 = c->n;
        // counter and records at the front of the workspace; no candidate -> job table (ONE query)
        const BatchTables t{nullptr, qbox, nullptr, nullptr, (int32_t*)workspace, (int32_t*)((char*)workspace + 256), nullptr, nullptr};
        a.grp_off = t.grp_off;
        a.grp_rec = t.grp_rec;
        if (int rc = launch_chunk_prep(a, t, nullptr, 1, c->n, stream)) return rc;
        return launch_pair_fused_chunk(a, chunk_items_bound(1, c->n, c->n), qbox, stream);
    }
    return dispatch_T(max_rows, [&](auto tc) -> int {
        constexpr int T = decltype(tc)::value;
        for (int64_t c0 = 0; c0 < c->n; c0 += cand_per_chunk) {
            a.cand0 = c0;
            a.cand1 = c0 + cand_per_chunk < c->n ? c0 + cand_per_chunk : c->n;
            const int64_t n_slots = (a.cand1 - a.cand0) * pairs_per_cand;
            const PairWs<T> ws = pair_ws_at<T>(workspace, n_slots);
            float* cbox = (float*)(((uintptr_t)(ws.diam2 + n_slots) + 15) & ~(uintptr_t)15);
            if constexpr (T == 1) {
                // a small pool of short documents (the per-query call of evaluate.py:58-76): one wave per pair, costs and solve in ONE
                // launch (pair_one_kernel) instead of the cost launch + the Sinkhorn launch and the workspace between them
                const int64_t groups4 = (a.cand1 - a.cand0 + 3) / 4 * (pairing == ASPIRE_PAIR_CROSS ? q->n : 1);
                const bool small_grid = !(pairing == ASPIRE_PAIR_CROSS && groups4 >= 2048);        // (beyond: the tiled cost kernel's grid)
                if (one_wave_form_ok(n_slots, q->ext == 0 && c->ext == 0 && !gram && !cost_only, small_grid)) {
                    if (int rc = launch_pair_one(a, n_slots, stream)) return rc;
                    continue;
                }
            }
            if (int rc = launch_cost_stage(a, T, q, c, ws.cost, ws.neg, ws.diam2, n_slots, qchunks, gram, qbox, cbox, c0 == 0, stream)) return rc;
            if (cost_only) continue;
            if (int rc = launch_sinkhorn_stage(a, T, ws.cost, ws.neg, ws.diam2, n_slots, max_rows, extra, 0, stream)) return rc;
        }
        return (int)ASPIRE_OK;
    });
}

// One otAspire call: the argument checks, the form by document length, the rank.
// Documents beyond the tile kernels' 32 rows: padded tensors that wide go through the one-workgroup-per-pair kernel
// (generic.hip) for every pair; CSR pools run the tile kernels with their documents' bound clamped to 32 rows (every pair
// of short documents is scored there, a pair that holds a longer one gets NaN) and the long-document kernel then rewrites
// exactly those pairs.  The rank follows.
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
    const int tile_max = 8 * kMaxT;
    // ONE_FORM (include/aspire_hip.h): every pair through the long-form kernel, whatever the size of the call
    const bool one_form = (prm->flags & ASPIRE_OT_FLAG_ONE_FORM) && !cost_only;
    if (max_rows_of(q, c) <= tile_max && !one_form) {
        if (int rc = ot_run_tiles(a, q, c, prm, workspace, workspace_bytes, s, cost_only)) return rc;
    } else {
        int skip = 0;
        if (q->ext == 0 && c->ext == 0 && !one_form) {      // (CSR: no pair outputs, `a` serves the tile kernels as it is)
            aspire_repset q32 = *q, c32 = *c;
            q32.max_len = q->max_len < tile_max ? q->max_len : tile_max;
            c32.max_len = c->max_len < tile_max ? c->max_len : tile_max;
            if (int rc = ot_run_tiles(a, &q32, &c32, prm, workspace, workspace_bytes, s, cost_only)) return rc;
            skip = tile_max;
        }
        if (cost_only) return ASPIRE_OK;
        const int rows_q = q->ext > 0 ? q->ext : q->max_len, rows_c = c->ext > 0 ? c->ext : c->max_len;
        if (int rc = launch_pair_generic(a, 0, skip, rows_q, rows_c, s)) return rc;
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
constexpr int kStagePrep = 1, kStageCost = 2, kStageSolve = 4, kStageRank = 8, kStageAll = 15;
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
    // Documents beyond the tile kernels' 32 rows (AspireNER's appended entity rows, models.py:224-233), as in ot_run: the tile
    // kernels run with their documents' bound clamped to 32 rows (a pair that holds a longer document gets NaN there) and the
    // long-document kernel (generic.hip) then rewrites exactly those pairs, in front of the rank.
    const int max_rows_all = max_rows_of(q, c);
    ASPIRE_REQUIRE(max_rows_all <= generic_max_rows(), ASPIRE_ERR_UNSUPPORTED,
                   "documents with more than %d sentence rows are not supported (got %d)", generic_max_rows(), max_rows_all);
    const int max_rows = max_rows_all < 8 * kMaxT ? max_rows_all : 8 * kMaxT;
    const BatchLayout L = batch_layout(J, C, max_rows, max_job, k);
    if (int rc = place_scratch(rank, workspace, workspace_bytes, L.total, L.topk, "aspire_ot_rank_batch_workspace_bytes")) return rc;
    const BatchTables t = batch_tables(workspace, L);
    if (!(stages & kStageRank)) rank.k = 0;      // (a stage mask of the debug entry point without the rank: scores only)
    ScoreArgs a{};
    fill_ot_args(a, q, c, kPairMapped, prm, nullptr, 0, want, scores);
    a.q_per_block = 1;
    fill_mapped_args(a, t, job_off, J, C, max_job);
    // Forms.  Small batches are latency bound and take the kernels the single-pool entry points use.  Once the batch fills
    // the chip (documents of <= 8 rows): the fused kernel -- four candidates of a job per wave, costs and solves in one
    // launch (fused.hip) -- or, pinned for A/B tests, the same cost kernel + the block Sinkhorn kernel as two launches.
    // (Chunks of jobs on two streams, Sinkhorn of chunk i beside the cost kernel of chunk i + 1, were measured and dropped:
    // 20 x 1000: 169 us on one stream, 213 / 266 / 403 us in 2 / 4 / 8 chunks -- cross-stream waits cost more than they hide.)
    if (prm->flags & ASPIRE_OT_FLAG_ONE_FORM) {
        // every pair through the long-form kernel (one workgroup per pair; it finds a candidate's job by searching job_off)
        a.qmap = nullptr;
        if (stages & kStageSolve)
            if (int rc = launch_pair_generic(a, 0, 0, q->max_len, c->max_len, s0)) return rc;
        return rank.rank(scores);
    }
    const int64_t groups_bound = J * ((max_job + 3) / 4);
    const int form_t = tuning().ot_form;
    const bool big = max_rows <= 8 && groups_bound >= kStreamMinGroupsBatch;
    const bool fused = max_rows <= 8 && (form_t == 3 || (form_t == 0 && big));
    a.tile_form = max_rows <= 8 && (form_t == 2 || fused);
    // Documents of up to 16 rows in a batch that fills the chip: usually pools of mostly short abstracts with a few longer
    // ones.  The fused kernel is queued in front of the 16-row streaming kernel + block Sinkhorn, and a census of the long
    // pairs, taken on the device, decides how they work (score_types.h: ScoreArgs::gate): few long pairs -- the fused kernel
    // scores the short ones, the 16-row kernels only the long ones; many -- the fused kernel returns at once.  No host round
    // trip, and ONE long document no longer moves 20 000 pairs onto kernels 2.5 x slower.
    const bool hybrid = max_rows > 8 && max_rows <= 16 && form_t == 0 && groups_bound >= 2048 && C >= 6000 && stages == kStageAll &&
                        prm->scaling >= 0.25 && want != ASPIRE_OT_PLAN_SIM && !tuning().fused_nosolve && !tuning().fused_valu &&
                        sinkhorn_form_honours_gate();
    // Short queries (facet-selected rows, models.py:127-163) against abstracts of up to 32 rows -- config 4's shape: the fused
    // kernel's CHUNK form, costs and solves of every pair in one launch behind a launch that sorts the candidates into items.
    const bool chunked = q->max_len <= 8 && max_rows > 8 && max_rows_all <= 8 * kMaxT && chunk_size_ok(C) && stages == kStageAll &&
                         prm->scaling >= 0.25 && !tuning().fused_valu;
    if (chunked) {
        if (int rc = launch_chunk_prep(a, t, job_off, J, max_job, s0)) return rc;
        if (int rc = launch_pair_fused_chunk(a, chunk_items_bound(J, C, max_job), t.qbox, s0)) return rc;
        return rank.rank(scores);
    }
    // Whole abstracts on both sides, documents of 17 .. 32 rows among them (un-faceted queries: pp_settings.py:2-3): the 16-row
    // streaming kernel on record items (a query half against two candidate halves) + the block Sinkhorn kernel on 24- / 32-row
    // workspace slots.  (Before: the VALU tile loop, one workgroup per candidate.)
    const bool rec16 = max_rows > 16 && max_rows_all <= 8 * kMaxT && chunk_size_ok(C) && stages == kStageAll && tuning().cost_path != 2;
    if (rec16) {
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
        return rank.rank(scores);
    }
    // batches of <= 64 jobs on the fused kernel need no tables launch: the kernel's waves derive them (fused.hip, SELF)
    const bool self = fused && fused_self_ok(J, prm);
    if ((stages & kStagePrep) && !self)
        if (int rc = launch_batch_tables(a, t, job_off, J, max_job, s0)) return rc;
    if (hybrid) {
        if (int rc = arm_long_pair_gate(a, t.gate, C, s0)) return rc;
        if (int rc = launch_pair_fused(a, groups_bound, t.qbox, s0)) return rc;
    }
    if (fused) {
        if (stages & (kStageCost | kStageSolve))
            if (int rc = launch_fused_form(a, groups_bound, self, stages == kStageAll, t.qbox, prm, s0)) return rc;
    } else {
        const int rc_run = dispatch_T(max_rows, [&](auto tc) -> int {
            constexpr int T = decltype(tc)::value;
            if constexpr (T == 1) {
                // a small batch of short documents: the single-pool calls' one-launch form (pair_one_kernel: one wave per pair) -- the
                // same kernel whether a pair is scored in a batch or in a call of its own: the same bits
                if (one_wave_form_ok(C, stages == kStageAll, !a.tile_form)) return launch_pair_one(a, C, s0);
            }
            const PairWs<T> ws = pair_ws_at<T>(t.slots, C);
            if (stages & kStageCost)
                if (int rc = launch_cost_stage(a, T, q, c, ws.cost, ws.neg, ws.diam2, C, 1, false, t.qbox, nullptr, true, s0)) return rc;
            if (stages & kStageSolve)
                if (int rc = launch_sinkhorn_stage(a, T, ws.cost, ws.neg, ws.diam2, C, max_rows, false, a.tile_form ? 3 : 0, s0)) return rc;
            return (int)ASPIRE_OK;
        });
        if (rc_run) return rc_run;
        if (max_rows_all > max_rows && (stages & kStageSolve))
            if (int rc = launch_pair_generic(a, 0, max_rows, q->max_len, c->max_len, s0)) return rc;
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
namespace {
// groups of four candidates from which aspire_l2max_rank_batch_f32 takes the streaming kernels (measured, tools/l2batchbench.py)
constexpr int64_t kL2StreamMinGroups = 384;
}  // namespace

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
    const bool one_form = (cdist_mode & ASPIRE_CDIST_ONE_FORM) != 0, center = (cdist_mode & ASPIRE_CDIST_CENTER) != 0;
    cdist_mode &= ~(ASPIRE_CDIST_ONE_FORM | ASPIRE_CDIST_CENTER);
    ScoreArgs a{};
    fill_set_args(a, q, c, kPairMapped);
    a.cdist_mode = cdist_mode;
    a.center = center;
    a.agg = ASPIRE_AGG_MAX;
    a.temp = 1.0;
    a.scores = scores;
    fill_mapped_args(a, t, job_off, J, C, max_job);
    const int64_t groups_bound = J * ((max_job + 3) / 4);
    const int form_t = tuning().ot_form;
    const bool big = groups_bound >= 2048 && C >= 6000 && form_t != 1;
    // (small batches too: a wave walks an item's twelve stages in ~15 us, what a one-workgroup-per-pair launch takes anyway)
    // short queries against abstracts of up to 32 rows (config 4's shape): the CHUNK items of ot_rank_batch, max epilogue
    if (q->max_len <= 8 && max_rows > 8 && max_rows <= 8 * kMaxT && chunk_size_ok(C) && !one_form) {
        if (int rc = launch_chunk_prep(a, t, job_off, J, max_job, s0)) return rc;
        if (int rc = launch_pair_fused_chunk_l2max(a, chunk_items_bound(J, C, max_job), s0)) return rc;
        return rank.rank(scores);
    }
    // whole abstracts of up to 32 rows against queries of 9 .. 16: the 16-row streaming kernel on record items, max epilogue (a
    // query of more than 16 rows would need its two halves' maxima joined across items: the per-candidate kernel keeps those)
    if (q->max_len <= 16 && max_rows > 16 && max_rows <= 8 * kMaxT && chunk_size_ok(C) && !one_form) {
        if (int rc = launch_rec_prep(a, t, job_off, J, max_job, s0)) return rc;
        if (int rc = launch_pair_tile16_rec_l2max(a, 2 * chunk_items_bound(J, C, max_job), s0)) return rc;
        return rank.rank(scores);
    }
    // batches of <= 64 jobs of short documents: the streaming kernel's waves derive the tables themselves (fused.hip, SELF) --
    // one launch in front of the rank, at any size (2 x 20: 19 us either way)
    const bool self = form_t != 1 && max_rows <= 8 && J <= 64 && !tuning().fused_noself && !one_form;
    const bool streaming = form_t != 1 && (self || big || form_t >= 2 || groups_bound >= kL2StreamMinGroups) && !one_form;
    if (!self)
        if (int rc = launch_batch_tables(a, t, job_off, J, max_job, s0)) return rc;
    // Forms: the streaming kernels once the batch fills the chip (documents of <= 8 rows: fused.hip's max-sim form, four
    // candidates of a job per wave; 9 .. 16 rows: tile16.hip, two), else -- small batches, longer documents -- the
    // one-workgroup-per-pair kernel (generic.hip).
    if (streaming && max_rows <= 8) {
        if (int rc = launch_pair_fused_l2max(a, groups_bound, s0, self)) return rc;
    } else if (streaming && max_rows <= 16) {
        // mostly short documents with a few of 9 .. 16 rows: the hybrid of ot_rank_batch (ScoreArgs::gate)
        if (big && form_t == 0) {
            if (int rc = arm_long_pair_gate(a, t.gate, C, s0)) return rc;
            if (int rc = launch_pair_fused_l2max(a, groups_bound, s0)) return rc;
        }
        if (int rc = launch_pair_tile16_l2max(a, 2 * groups_bound, s0)) return rc;
    } else if (max_rows <= 8 * kMaxT && !one_form) {
        // one workgroup per candidate against its job's query (small batches, documents of 17 .. 32 rows)
        if (int rc = launch_l2max_tiles(a, max_rows, 1, s0)) return rc;
    } else {
        if (int rc = launch_pair_generic(a, 1, 0, q->max_len, c->max_len, s0)) return rc;
    }
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
