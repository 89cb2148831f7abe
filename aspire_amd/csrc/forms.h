// Which kernel family scores a call: the decisions of the four scoring entry families and of the two stages that run on workspace
// slots, as pure functions of the host fields of the rep sets, of what the call asked for and of tuning() (forms.hip holds every
// rule and every threshold).  Nothing here launches, allocates or formats; score.hip switches over the plans, cost_valu.hip and
// sinkhorn.hip over the stage choices.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "common.h"

namespace aspire {

// stages of a batched otAspire call (the debug entry point's mask)
constexpr int kStagePrep = 1, kStageCost = 2, kStageSolve = 4, kStageRank = 8, kStageAll = 15;
// rows of a tile side of the kernels that run on workspace slots (8 * kMaxT of score_types.h): longer documents go to generic.hip
constexpr int kTileMaxRows = 32;
// candidate rows of a Gram tile (gram.hip: kBM)
constexpr int kGramCandRows = 128;

enum class Form {
    None,          // nothing to launch (the cost stage alone of a call the long-document kernel scores)
    Generic,       // generic.hip: one workgroup per pair, every pair
    GramPlanes,    // gramp.hip: the fp16-plane tiles, whatever the number of queries
    Gram,          // gram.hip: the matrix-core tiles (max-sim: one launch; otAspire: Tiles with ScorePlan::gram)
    Stream16,      // tile16.hip: the 16-row streaming kernel's max-sim form
    FusedStream,   // fused.hip: the streaming phase with the max epilogue (max-sim, tables or CROSS)
    FusedInbox,    // fused.hip: ONE query, the kernel forms its box itself
    FusedQbox,     // fused.hip: query boxes from a launch in front (or the caller's diameters)
    FusedSelf,     // fused.hip: batches of <= 64 jobs, the waves derive the tables
    FusedTables,   // fused.hip: batches on the tables of batch_prep.hip
    Chunk,         // fused.hip on CHUNK items: short queries against documents of up to 32 rows
    Rec16,         // tile16.hip on REC items (+ the block solver for otAspire)
    OneWave,       // sinkhorn.hip: pair_one_kernel, costs and solve of a short pair in one wave
    Tiles,         // max-sim: l2max_kernel; otAspire: the cost stage + the solve stage on workspace slots
    Hybrid,        // the fused kernel queued in front of the 16-row kernels behind the long-pair gate (ScoreArgs::gate)
};

struct ScorePlan {
    Form form;
    int max_rows;         // the row bound the tile kernels use (clamped to kTileMaxRows for CSR sets with longer documents)
    bool then_generic;    // ... and the long-document kernel then rewrites the pairs that hold a longer one
    bool gram;            // otAspire Tiles: the cost stage on the Gram tiles
    bool cost_from_neg;   // ... which then stores -cdist only (ScoreArgs::cost_from_neg)
    bool qbox_first;      // FusedQbox: a doc_box launch over the queries goes first
    bool tables_first;    // batched: launch_batch_tables goes first
    bool tile_form;       // batched otAspire: ScoreArgs::tile_form
};

// what an otAspire call asked for beyond its sets and parameters
struct OtAsked {
    bool pair_outputs, caller_diameters, cost_only, has_workspace;
    size_t workspace_bytes;
};

int max_rows_of(const aspire_repset* q, const aspire_repset* c);
// a CSR set as the tile kernels are to see it: its documents' bound clamped to kTileMaxRows (a pair that holds a longer document
// gets NaN there and is rewritten by the long-document kernel)
inline aspire_repset tile_bound_set(const aspire_repset* s) {
    aspire_repset r = *s;
    if (s->ext == 0 && r.max_len > kTileMaxRows) r.max_len = kTileMaxRows;
    return r;
}
int gram_slot_rows(int max_len);
// bytes at the tail of a per-call otAspire workspace that hold the queries' boxes
inline size_t qbox_bytes(const aspire_repset* q) { return (size_t)q->n * 2 * kD * sizeof(float); }
// the per-call workspace sizing asks this too (a candidate's box on the matrix-core path)
bool gram_path_wanted(const aspire_repset* q, const aspire_repset* c, int pairing);

// ---- one decision per entry family ----
// max-sim per call (aspire_l2agg_scores_f32)
ScorePlan plan_l2agg(const aspire_repset* q, const aspire_repset* c, int pairing, int agg, bool pair_outputs, bool one_form);
// otAspire per call (ot_run); a Tiles plan decides per candidate chunk whether the chunk takes the one-wave form
ScorePlan plan_ot(const aspire_repset* q, const aspire_repset* c, int pairing, const aspire_ot_params* prm, const OtAsked& asked);
bool ot_chunk_one_wave(const ScorePlan& plan, const aspire_repset* q, const aspire_repset* c, int pairing, int64_t chunk_cands,
                       bool cost_only);
// otAspire batched (ot_rank_batch)
ScorePlan plan_ot_batch(const aspire_repset* q, const aspire_repset* c, int64_t max_job, const aspire_ot_params* prm, int want,
                        int stages);
// max-sim batched (aspire_l2max_rank_batch_f32)
ScorePlan plan_l2max_batch(const aspire_repset* q, const aspire_repset* c, int64_t max_job, bool one_form);

// ---- the stages on workspace slots ----
enum class CostKernel { Gram, Tile, Cost1, Tile16, Cost1Sub, Cost };
struct CostChoice {
    CostKernel kernel;
    int64_t items;      // Tile: groups of four candidates x queries; Tile16: pairs of candidates x queries; Cost1Sub: 8 x 8 sub-tiles
};
// T: tiles a side; chunk_cands: a.cand1 - a.cand0; MAPPED pairing: jobs x max_job_groups bounds the groups, tables_built = a.grp_off
CostChoice cost_kernel_form(int T, const aspire_repset* q, const aspire_repset* c, int pairing, bool gram, bool tile_form,
                            bool tables_built, int64_t chunk_cands, int64_t jobs, int64_t max_job_groups, int64_t n_slots);

enum class Solver { Wave, Block };
struct SolveChoice {
    Solver kernel;
    int lanes, per_lane;      // Block: lanes per pair side and entries per lane side (sinkhorn_block_kernel<T, LD, R>)
    bool repair;              // Block: sinkhorn_repair_kernel follows
};
// form_hint: 3 where the caller's form needs the block kernels (batches on the throughput kernels, REC), else 0
SolveChoice solver_form(int T, int64_t n_slots, int max_rows, bool pair_outputs, int form_hint);

}  // namespace aspire
