// Preparation kernels: the tables of batched jobs (J independent (query, pool) re-ranks in one call) and the items of the
// CHUNK / REC forms, which the single-pool calls take too.  Each is one small launch in front of a scoring launch of fused.hip or
// tile16.hip, which reads what it wrote (score_types.h: ScoreArgs::grp_rec and its neighbours).
//
// Host side (the end of the file): the bound on the items a launch can make, which sizes the callers' workspaces, and one launcher
// per kernel; all declared in score_types.h.
#include "common.h"
#include "score_types.h"
#include "score_device.h"

namespace aspire {
namespace {

// One workgroup per job j: the per-coordinate box of query j (the cost kernel adds each candidate's rows to it), the
// job's first group of four (groups never straddle jobs, so a wave of the cost kernel serves ONE query), and the
// candidate -> job / group -> job tables the kernels index.
__global__ void __launch_bounds__(192) batch_prep_kernel(RepSet q, RepSet c, const int32_t* __restrict__ job_off, int J,
                                                         float* __restrict__ qbox, int32_t* __restrict__ cand_job,
                                                         int32_t* __restrict__ grp_off, int32_t* __restrict__ grp_job,
                                                         int32_t* __restrict__ grp_rec) {
    // grid = (J, parts + 1): block (j, parts) forms the query's box and nothing else -- its chain of dependent loads (length,
    // start -> rows -> store) runs beside the table blocks' chain instead of in front of it; every other part of a job derives
    // the job's first group itself (a block-wide sum over the earlier jobs' group counts) and then takes its share of the
    // job's candidates / groups.  (One block per job made 20 blocks walk 250 groups each with dependent gathers: 20 us for
    // a 20 x 1000 batch.)
    __shared__ int part[3];
    const int j = blockIdx.x, tid = threadIdx.x;
    if (blockIdx.y == gridDim.y - 1) {
        const int n = q.len[j];
        const float* doc = q.rows + (size_t)q.start[j] * kD + tid * 4;
        float4 mn, mx;
        doc_box_chunk(doc, n, mn, mx);
        *reinterpret_cast<float4*>(qbox + (size_t)j * 2 * kD + tid * 4) = mn;
        *reinterpret_cast<float4*>(qbox + (size_t)j * 2 * kD + kD + tid * 4) = mx;
        return;
    }
    const int sub = blockIdx.y * 192 + tid, nsub = (gridDim.y - 1) * 192;
    int g = 0;
    for (int i = tid; i < j; i += 192) g += (job_off[i + 1] - job_off[i] + 3) >> 2;
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) g += __shfl_xor(g, m);
    if ((tid & 63) == 0) part[tid >> 6] = g;
    __syncthreads();
    const int g0 = part[0] + part[1] + part[2];
    const int c0 = job_off[j], c1 = job_off[j + 1], ng = (c1 - c0 + 3) >> 2;
    if (blockIdx.y == 0 && tid == 0) {
        grp_off[j] = g0;
        if (j == J - 1) grp_off[J] = g0 + ng;
    }
    for (int cc = c0 + sub; cc < c1; cc += nsub) cand_job[cc] = j;
    for (int k = sub; k < ng; k += nsub) grp_job[g0 + k] = j;
    // the per-group records of the fused kernel (see ScoreArgs::grp_rec): thread = (group, field)
    const int q_len = q.len[j], q_start = q.start[j];
    for (int e = sub; e < ng * 16; e += nsub) {
        const int k = e >> 4, f = e & 15;
        const int first = c0 + 4 * k;
        const int cand = min(first + (f & 3), c1 - 1);
        int v;
        if (f == 0) v = j;
        else if (f == 1) v = q_len;
        else if (f == 2) v = q_start;
        else if (f == 3) v = min(4, c1 - first);
        else if (f < 8) v = cand;
        else if (f < 12) v = c.len[cand];
        else v = c.start[cand];
        grp_rec[(size_t)(g0 + k) * 16 + f] = v;
    }
}

// Items of the fused kernel's CHUNK form (fused.hip) for batched jobs whose candidates reach 9 .. 32 rows: an item = four 8-row
// chunk slots holding candidates of ONE job with [4], [3, 1], [2, 2], [2, 1, 1] or [1, 1, 1, 1] chunks (a 2-chunk candidate on
// slots 0, 1 or 2, 3; a 3-chunk one on 0 .. 2 with a 1-chunk candidate beside it: on the config-4 shape 3300 -> 2950 items, so
// that no SIMD of the scoring launch holds two waves of two items each).  Block (j, part) counts its slice of job j's candidates
// by chunk count (LDS counters), reserves its items with ONE atomicAdd on the launch's item counter (items need not be
// contiguous per job: a score is stored by candidate index), gives every candidate its place by its rank within its class, and
// writes the 64-byte item records: [0] query, [1] its len, [2] its first row, [3] widest exchange across lane groups the item
// needs (1, 2, 4), [4..7] the slots' candidates, [8..11] per slot: len | first slot of the candidate << 8 | its slots << 12 |
// real << 16, [12..15] the slots' first rows.  Slots that stay empty repeat the item's first candidate as a one-chunk
// candidate (scored, never stored).  Block (j, last) forms the query's box, as in batch_prep_kernel.
constexpr int kChunkPrepPart = 384;      // candidates per classification block
// job_off == nullptr: ONE query against the pool [0, c.n) (the single-pool entry points); cand_job may be null then.
// region_cap > 0 (at most 64 slices): no counter -- slice s = j * parts + part leaves its item count in counter[s] and its records in
// records [s * region_cap, ..) (ScoreArgs::chunk_regions).
__global__ void __launch_bounds__(192) chunk_prep_kernel(RepSet q, RepSet c, const int32_t* __restrict__ job_off, float* __restrict__ qbox,
                                                         int32_t* __restrict__ cand_job, int32_t* __restrict__ counter,
                                                         int32_t* __restrict__ grp_rec, int region_cap) {
    __shared__ int cnt[4], pos[4], base_s;
    const int slice = blockIdx.x * (gridDim.y - 1) + blockIdx.y;
    const int j = blockIdx.x, tid = threadIdx.x;
    if (blockIdx.y == gridDim.y - 1) {
        const int n = q.len[j];
        const float* doc = q.rows + (size_t)q.start[j] * kD + tid * 4;
        float4 mn, mx;
        doc_box_chunk(doc, n, mn, mx);
        *reinterpret_cast<float4*>(qbox + (size_t)j * 2 * kD + tid * 4) = mn;
        *reinterpret_cast<float4*>(qbox + (size_t)j * 2 * kD + kD + tid * 4) = mx;
        return;
    }
    const int c0 = (job_off ? job_off[j] : 0) + blockIdx.y * kChunkPrepPart, c1 = min(job_off ? job_off[j + 1] : (int)c.n, c0 + kChunkPrepPart);
    if (c0 >= c1) {
        if (region_cap > 0 && tid == 0) counter[slice] = 0;
        return;
    }
    if (tid < 4) cnt[tid] = pos[tid] = 0;
    __syncthreads();
    int len[2], start[2], nch[2];
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const int cc = c0 + tid + 192 * r;
        len[r] = cc < c1 ? c.len[cc] : 0;
        start[r] = cc < c1 ? c.start[cc] : 0;
        nch[r] = min(4, max(1, (len[r] + 7) >> 3));          // chunks (a longer document is poisoned by the kernel)
        if (cc < c1) {
            atomicAdd(&cnt[nch[r] - 1], 1);
            if (cand_job) cand_job[cc] = j;
        }
    }
    __syncthreads();
    // the block's items, in this order: [4] x n4, [3, 1] x n3, [2, 2] x n2 / 2, one [2, 1, 1] if n2 is odd, [1, 1, 1, 1] for the
    // singles the [3, 1] and [2, 1, 1] items have left
    const int n1 = cnt[0], n2 = cnt[1], n3 = cnt[2], n4 = cnt[3];
    const int s3 = min(n1, n3);                               // singles beside 3-chunk candidates
    const int odd2 = n2 & 1, s2 = odd2 ? min(n1 - s3, 2) : 0; // singles beside the odd 2-chunk candidate
    const int n1r = n1 - s3 - s2, items1 = (n1r + 3) >> 2;
    if (tid == 0) {
        const int items = n4 + n3 + (n2 >> 1) + odd2 + items1;
        if (region_cap > 0) {
            counter[slice] = items;
            base_s = slice * region_cap;
        } else {
            base_s = atomicAdd(counter, items);
        }
    }
    __syncthreads();
    const int b4 = base_s, b3 = b4 + n4, b2 = b3 + n3, bo = b2 + (n2 >> 1), b1 = bo + odd2;
    const int q_len = q.len[j], q_start = q.start[j];
    auto put = [&](int item, int slot, int cc, int ln, int st, int g0, int gsz, int real) {
        int32_t* rec = grp_rec + (size_t)item * 16;
        rec[4 + slot] = cc;
        rec[8 + slot] = ln | (g0 << 8) | (gsz << 12) | (real << 16);
        rec[12 + slot] = st;
    };
    auto head = [&](int item, int w) {
        int32_t* rec = grp_rec + (size_t)item * 16;
        rec[0] = j;
        rec[1] = q_len;
        rec[2] = q_start;
        rec[3] = w;
    };
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const int cc = c0 + tid + 192 * r;
        if (cc >= c1) continue;
        const int k = nch[r], ps = atomicAdd(&pos[k - 1], 1), ln = len[r], st = start[r];
        if (k == 4) {
            for (int t = 0; t < 4; ++t) put(b4 + ps, t, cc, ln, st, 0, 4, 1);
            head(b4 + ps, 4);
        } else if (k == 3) {
            for (int t = 0; t < 3; ++t) put(b3 + ps, t, cc, ln, st, 0, 3, 1);
            if (ps >= s3) put(b3 + ps, 3, cc, ln, st, 3, 1, 0);             // no single left for this item
            head(b3 + ps, 4);
        } else if (k == 2) {
            const bool last_odd = odd2 && ps == n2 - 1;
            const int item = last_odd ? bo : b2 + (ps >> 1), s0 = last_odd ? 0 : 2 * (ps & 1);
            put(item, s0, cc, ln, st, s0, 2, 1);
            put(item, s0 + 1, cc, ln, st, s0, 2, 1);
            if (s0 == 0) head(item, 2);
            if (last_odd)
                for (int t = 2 + s2; t < 4; ++t) put(item, t, cc, ln, st, t, 1, 0);
        } else if (ps < s3) {
            put(b3 + ps, 3, cc, ln, st, 3, 1, 1);
        } else if (ps < s3 + s2) {
            put(bo, 2 + (ps - s3), cc, ln, st, 2 + (ps - s3), 1, 1);
        } else {
            const int rr = ps - s3 - s2, item = b1 + (rr >> 2), slot = rr & 3;
            put(item, slot, cc, ln, st, slot, 1, 1);
            if (slot == 0) {
                head(item, 1);
                for (int t = min(4, n1r - (rr & ~3)); t < 4; ++t) put(item, t, cc, ln, st, t, 1, 0);
            }
        }
    }
}
// Items of the 16-row streaming kernel's REC form (tile16.hip) for batched jobs whose queries AND candidates can have 9 .. 32 rows:
// an item = a 16-row half of the query against two candidate slots of 16 rows -- two candidates of <= 16 rows, or the two halves
// of one candidate of 17 .. 32.  Same scheme as chunk_prep_kernel (counts in LDS, one atomicAdd on the launch's item counter per
// block, a candidate's place by its rank within its class); a query of more than 16 rows gets every item twice, once per half.
// Record: [0] query, [1] its len, [2] its first row, [3] query half | wide << 8, [4,5] the slots' candidates, [6,7] their lens,
// [8,9] their first rows, [10,11] first row of the slot's half (0 / 16), [12,13] real.
__global__ void __launch_bounds__(192) chunk16_prep_kernel(RepSet q, RepSet c, const int32_t* __restrict__ job_off, float* __restrict__ qbox,
                                                           int32_t* __restrict__ cand_job, int32_t* __restrict__ counter,
                                                           int32_t* __restrict__ grp_rec) {
    __shared__ int cnt[2], pos[2], base_s;
    const int j = blockIdx.x, tid = threadIdx.x;
    if (blockIdx.y == gridDim.y - 1) {
        const int n = q.len[j];
        const float* doc = q.rows + (size_t)q.start[j] * kD + tid * 4;
        float4 mn, mx;
        doc_box_chunk(doc, n, mn, mx);
        *reinterpret_cast<float4*>(qbox + (size_t)j * 2 * kD + tid * 4) = mn;
        *reinterpret_cast<float4*>(qbox + (size_t)j * 2 * kD + kD + tid * 4) = mx;
        return;
    }
    const int c0 = job_off[j] + blockIdx.y * kChunkPrepPart, c1 = min(job_off[j + 1], c0 + kChunkPrepPart);
    if (c0 >= c1) return;
    if (tid < 2) cnt[tid] = pos[tid] = 0;
    __syncthreads();
    int len[2], start[2];
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const int cc = c0 + tid + 192 * r;
        len[r] = cc < c1 ? c.len[cc] : 0;
        start[r] = cc < c1 ? c.start[cc] : 0;
        if (cc < c1) {
            atomicAdd(&cnt[len[r] > 16 ? 1 : 0], 1);
            cand_job[cc] = j;
        }
    }
    __syncthreads();
    const int q_len = q.len[j], q_start = q.start[j], nqh = q_len > 16 ? 2 : 1;
    const int n_narrow = cnt[0], n_wide = cnt[1], per_half = ((n_narrow + 1) >> 1) + n_wide;
    if (tid == 0) base_s = atomicAdd(counter, nqh * per_half);
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const int cc = c0 + tid + 192 * r;
        if (cc >= c1) continue;
        const bool wide = len[r] > 16;
        const int ps = atomicAdd(&pos[wide ? 1 : 0], 1);
        const int local = wide ? ((n_narrow + 1) >> 1) + ps : ps >> 1, slot = wide ? 0 : ps & 1;
        const bool alone = !wide && slot == 0 && ps == n_narrow - 1;      // an odd narrow candidate: its item's second slot repeats it
        for (int qh = 0; qh < nqh; ++qh) {
            int32_t* rec = grp_rec + (size_t)(base_s + qh * per_half + local) * 16;
            if (slot == 0) {
                rec[0] = j;
                rec[1] = q_len;
                rec[2] = q_start;
                rec[3] = qh | (wide ? 256 : 0);
            }
            for (int t = slot; t < (wide || alone ? 2 : slot + 1); ++t) {
                rec[4 + t] = cc;
                rec[6 + t] = len[r];
                rec[8 + t] = start[r];
                rec[10 + t] = wide ? 16 * t : 0;
                rec[12 + t] = (wide || t == slot) ? 1 : 0;
            }
        }
    }
}

// ---- host side of the preparation kernels: sizes and launches -------------------------------------------------------------
// parts (classification blocks) per job, and the bound on the items the launch can make
int64_t chunk_parts(int64_t max_job) { return max_job > 0 ? (max_job + kChunkPrepPart - 1) / kChunkPrepPart : 1; }
// CHUNK items without a counter (ScoreArgs::chunk_regions): slices = J * parts <= 64; a slice's region holds min(384, max_job) records
int chunk_regions_of(int64_t J, int64_t max_job) {
    const int64_t n = J * chunk_parts(max_job);
    return n <= 64 ? (int)n : 0;
}
int chunk_region_cap_of(int64_t max_job) { return (int)(max_job < 384 ? (max_job > 0 ? max_job : 1) : 384); }
}  // namespace

int64_t chunk_items_bound(int64_t J, int64_t C, int64_t max_job) {
    const int64_t by_count = C + 3 * J * chunk_parts(max_job);
    const int64_t by_region = (int64_t)chunk_regions_of(J, max_job) * chunk_region_cap_of(max_job);      // (regions mode: every slice its own region)
    return by_count > by_region ? by_count : by_region;
}

// The tables of a batch on the groups-of-four kernels: batch_prep_kernel fills t.qbox, t.cand_job, t.grp_off, t.grp_job, t.grp_rec.
int launch_batch_tables(const ScoreArgs& a, const BatchTables& t, const int32_t* job_off, int64_t J, int64_t max_job, hipStream_t s) {
    // parts per job: enough blocks that a job's groups take a couple of trips each
    const int64_t work = ((max_job + 3) / 4) * 16;
    int64_t parts = (work + 2 * 192 - 1) / (2 * 192);
    parts = parts < 1 ? 1 : parts > 64 ? 64 : parts;
    while (parts > 1 && J * parts > 4096) parts /= 2;
    hipLaunchKernelGGL(batch_prep_kernel, dim3((unsigned)J, (unsigned)parts + 1), dim3(192), 0, s, a.q, a.c, job_off, (int)J, t.qbox, t.cand_job,
                       t.grp_off, t.grp_job, t.grp_rec);
    ASPIRE_LAUNCH_OK();
    return ASPIRE_OK;
}
// The items of the CHUNK form (chunk_prep_kernel): records into t.grp_rec, their count(s) into t.grp_off, the queries' boxes into
// t.qbox; sets a.chunk_regions / a.chunk_region_cap for the scoring launch.  The single-pool caller passes job_off = nullptr, J = 1,
// max_job = the pool (t.cand_job may be null then).
int launch_chunk_prep(ScoreArgs& a, const BatchTables& t, const int32_t* job_off, int64_t J, int64_t max_job, hipStream_t s) {
    a.chunk_regions = chunk_regions_of(J, max_job);
    a.chunk_region_cap = chunk_region_cap_of(max_job);
    if (a.chunk_regions == 0) ASPIRE_HIP_OK(hipMemsetAsync(t.grp_off, 0, sizeof(int32_t), s));
    hipLaunchKernelGGL(chunk_prep_kernel, dim3((unsigned)J, (unsigned)chunk_parts(max_job) + 1), dim3(192), 0, s, a.q, a.c, job_off, t.qbox,
                       t.cand_job, t.grp_off, t.grp_rec, a.chunk_regions > 0 ? a.chunk_region_cap : 0);
    ASPIRE_LAUNCH_OK();
    return ASPIRE_OK;
}
// The items of the REC form (chunk16_prep_kernel), counted in t.grp_off[0].
int launch_rec_prep(const ScoreArgs& a, const BatchTables& t, const int32_t* job_off, int64_t J, int64_t max_job, hipStream_t s) {
    ASPIRE_HIP_OK(hipMemsetAsync(t.grp_off, 0, sizeof(int32_t), s));
    hipLaunchKernelGGL(chunk16_prep_kernel, dim3((unsigned)J, (unsigned)chunk_parts(max_job) + 1), dim3(192), 0, s, a.q, a.c, job_off, t.qbox,
                       t.cand_job, t.grp_off, t.grp_rec);
    ASPIRE_LAUNCH_OK();
    return ASPIRE_OK;
}

}  // namespace aspire
