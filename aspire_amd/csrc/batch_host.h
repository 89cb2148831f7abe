// Host side that the six batched rank entry points share (score.hip: aspire_ot_rank_batch_f32, aspire_l2max_rank_batch_f32;
// l2agg_pair.hip: aspire_l2agg_rank_batch_f32; dotmax.hip: aspire_dotmax_rank_batch_f32; jointsm.hip:
// aspire_jointsm_rank_batch_f32; dense.hip: aspire_dense_rank_batch_f32): the argument checks every one of them makes after its
// own set check, the workspace check behind them, the workspace size of the four that need the rank's scratch only, and the rank
// that ends every one of them.  Host only: no kernel, nothing a kernel reads.
#pragma once
#include "common.h"
#include "topk_device.h"

namespace aspire {

// The rank tail of a batched call: per-job top-k lists of the segmented scores (topk_run with seg_off = job_off), on the
// call's stream behind the scoring kernels.  k == 0: scores only, rank() does nothing.
struct BatchRank {
    int64_t J, max_job, k;
    float* top_scores;
    int64_t* top_idx;
    uint64_t* keys;
    const int32_t* job_off;
    const int32_t* job_base;
    void* stream;
    void* scratch = nullptr;       // the rank's multi-pass scratch (aspire_topk_workspace_bytes; none for short pools)
    size_t scratch_bytes = 0;

    int rank(const float* scores) const {
        if (k <= 0) return ASPIRE_OK;
        return topk_run(scores, J, max_job, k, 0, keys ? nullptr : top_scores, keys ? nullptr : top_idx, keys, scratch, scratch_bytes,
                        stream, job_off, job_base);
    }
};

// The workspace check of an entry whose `query_fn` asks for `need` bytes, and the rank's scratch placed `scratch_off` bytes into it.
// A null workspace passes only where nothing is needed: never for the OT and l2max layouts (score.hip), which hold a gate word.
static int place_scratch(BatchRank& r, void* workspace, size_t workspace_bytes, size_t need, size_t scratch_off, const char* query_fn) {
    ASPIRE_REQUIRE(workspace_bytes >= need && (need == 0 || workspace), ASPIRE_ERR_INVALID_ARG,
                   "workspace too small: %zu bytes given, %s says %zu", workspace_bytes, query_fn, need);
    ASPIRE_REQUIRE(((uintptr_t)workspace & 15) == 0, ASPIRE_ERR_INVALID_ARG, "workspace must be 16-byte aligned");
    r.scratch_bytes = aspire_topk_workspace_bytes(r.J, r.max_job, r.k);
    r.scratch = r.scratch_bytes ? (char*)workspace + scratch_off : nullptr;
    return ASPIRE_OK;
}

// The workspace of an entry that needs the rank's scratch and nothing else (l2agg, dotmax, jointsm, dense)
inline size_t rank_scratch_only_bytes(int64_t J, int64_t C, int64_t max_job, int64_t k) {
    if (J <= 0 || C <= 0 || k <= 0) return 0;
    return aspire_topk_workspace_bytes(J, max_job, k);
}
inline size_t rank_scratch_only_bytes(const aspire_repset* q, const aspire_repset* c, int64_t max_job, int64_t k) {
    return q && c ? rank_scratch_only_bytes(q->n, c->n, max_job, k) : 0;
}

// What a batched entry point checks once its rep sets are known to be sound (check_repsets / check_dot_sets).  `go_on` false:
// the call is finished -- an argument error, no jobs, or only empty pools (the lists are all padding) -- and the entry point
// returns the code; true: C > 0 candidates to score into `scores`, then `r.rank(scores)`.
inline int batch_preamble(const aspire_repset* q, const aspire_repset* c, float* scores, BatchRank& r, bool& go_on) {
    go_on = false;
    const int64_t J = q->n, C = c->n;
    ASPIRE_REQUIRE(q->ext == 0 && c->ext == 0, ASPIRE_ERR_INVALID_ARG, "batched jobs take CSR rep sets (ext == 0)");
    ASPIRE_REQUIRE(r.k >= 0 && (r.k == 0 || (r.top_scores && r.top_idx) || r.keys), ASPIRE_ERR_INVALID_ARG,
                   "k > 0 needs (top_scores, top_idx) or keys");
    if (J == 0) return ASPIRE_OK;
    ASPIRE_REQUIRE(r.job_off && r.max_job >= 0 && r.max_job <= C, ASPIRE_ERR_INVALID_ARG, "need job_off and 0 <= max_job <= C");
    ASPIRE_REQUIRE(J < ((int64_t)1 << 30) && C < ((int64_t)1 << 31) - 8, ASPIRE_ERR_UNSUPPORTED, "batch too large for 32-bit offsets");
    if (C == 0) {
        // every pool is empty (max_job == 0 too): the lists are all padding, no scratch
        return r.rank(reinterpret_cast<const float*>(r.job_off));     // every segment is empty: never dereferenced
    }
    ASPIRE_REQUIRE(scores, ASPIRE_ERR_INVALID_ARG, "null scores");
    go_on = true;
    return ASPIRE_OK;
}

}  // namespace aspire
