// The embedding lookup under training (include/aspire_hip.h: aspire_bert_embed_sum_f32, aspire_bert_embed_backward_f32): BertEmbeddings'
// sum in front of the training layer stack and the three tables' gradients behind its backward.  Rows of 768 in enc_rows.hip's layout:
// one wave per row, a lane holds three 16-byte pieces (d = 4 lane + 256 c; pair_bwd.h's Row), 16-byte loads and stores.
//
// Kernels
//   embed_sum_kernel         out[m] = (word[tok[m]] + type[typ[m]]) + pos[m % L]; NaN for an id or type out of range
//                                                                                                          (one wave per token row)
//   embed_rank_kernel        rank of the key (tok[m], m) among all M keys by counting the keys below it, the ids staged through LDS in
//                            tiles of kRankTile; order[rank] = m, sorted[rank] = tok[m] (an id out of range sorts as `vocab`, behind
//                            every table row)                                                                (one thread per token)
//   embed_word_grad_kernel   table row v: lower bound of v in sorted (wave-uniform), then the run's gradient rows added in run order =
//                            ascending m, kRunLoads row loads in flight; the row, or zeros, written once
//                                                                                  (one wave per table row, grid-strided over vocab)
//   embed_pos_grad_kernel    position row l: the B rows grad[b, l] added in ascending b; zeros for l >= L     (one wave per table row)
//   embed_type_grad_kernel   type row t, 16 columns per workgroup: thread group j adds the rows of type t among rows [j R, (j + 1) R),
//                            R = ceil(M / 64), ascending; the 64 partials meet in LDS and are added ascending
//                                                                                          (one workgroup per (16 columns, type))
// No atomics and no zero-fill: every output element has one writer and every sum a fixed order, so two runs give the same bits.
#include <limits.h>

#include "pair_bwd.h"

namespace aspire {
namespace {

constexpr int kRankTile = 1024;             // ids staged in LDS per step of the rank pass
constexpr int64_t kEmbedMaxRows = 65536;    // token rows the rank pass serves (M^2 compares: 4.3e9 there)
constexpr int kRunLoads = 8;                // gradient rows in flight per wave of the word-table kernel
constexpr int kTypeParts = 64;              // partial sums per (type, column) of the type-table kernel
constexpr int kTypeCols = 16;               // columns per workgroup there
constexpr int kMaxGrid = 2048;              // workgroups of the grid-strided word-table kernel

// pair_bwd.h's Row: a lane's 12 coordinates of a row (4 lane + 256 k + (0 .. 3)), three 16-byte pieces
__device__ __forceinline__ void add_row(Row& acc, const Row& r) {
    acc.x += r.x;
    acc.y += r.y;
    acc.z += r.z;
}

__global__ void __launch_bounds__(256) embed_sum_kernel(const float* __restrict__ word, const float* __restrict__ pos,
                                                        const float* __restrict__ type_emb, const int64_t* __restrict__ tok,
                                                        const int64_t* __restrict__ typ, int64_t rows, int64_t L, int64_t vocab,
                                                        int64_t n_types, float* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int64_t t = tok[row], ty = typ ? typ[row] : 0, p = row % L;       // (p < L <= max_pos: the host checked)
    Row o = splat(__builtin_nanf(""));
    if (t >= 0 && t < vocab && ty >= 0 && ty < n_types) {
        const Row a = load_row(word + t * kD, lane), b = load_row(type_emb + ty * kD, lane), e = load_row(pos + p * kD, lane);
        o = Row{(a.x + b.x) + e.x, (a.y + b.y) + e.y, (a.z + b.z) + e.z};        // BertEmbeddings: (word + type) + position
    }
    store_row(out + row * kD, lane, o);
}

// the sort key of token j: its id, or `vocab` for an id that names no table row (vocab < INT_MAX: the host checked)
__device__ __forceinline__ int embed_key(const int64_t* __restrict__ tok, int j, int vocab) {
    const int64_t t = tok[j];
    return t >= 0 && t < vocab ? (int)t : vocab;
}

// MODE 0: every staged index lies below every token of the workgroup (a tie counts), 2: above (a tie does not), 1: compare the indices
template <int MODE>
__device__ __forceinline__ int count_below(const int* keys, int j0, int mine, int m) {
    int n = 0;
#pragma unroll 8
    for (int j = 0; j < kRankTile; j += 4) {
        const int4 k = *reinterpret_cast<const int4*>(keys + j);
        if constexpr (MODE == 0) {
            n += (k.x <= mine) + (k.y <= mine) + (k.z <= mine) + (k.w <= mine);
        } else if constexpr (MODE == 2) {
            n += (k.x < mine) + (k.y < mine) + (k.z < mine) + (k.w < mine);
        } else {
            const int i = j0 + j;
            n += (k.x < mine || (k.x == mine && i < m)) + (k.y < mine || (k.y == mine && i + 1 < m)) +
                 (k.z < mine || (k.z == mine && i + 2 < m)) + (k.w < mine || (k.w == mine && i + 3 < m));
        }
    }
    return n;
}

// The keys (id, m) are distinct and totally ordered, so the ranks are a permutation of 0 .. M - 1: every slot of order / sorted has one
// writer and lies inside the arrays.
__global__ void __launch_bounds__(256) embed_rank_kernel(const int64_t* __restrict__ tok, int M, int vocab, int* __restrict__ order,
                                                         int* __restrict__ sorted) {
    __shared__ __attribute__((aligned(16))) int keys[kRankTile];
    const int m0 = blockIdx.x * 256, m = m0 + threadIdx.x;
    const int mine = m < M ? embed_key(tok, m, vocab) : 0;
    int rank = 0;
    for (int j0 = 0; j0 < M; j0 += kRankTile) {
        __syncthreads();        // the tile is read no more
        for (int j = threadIdx.x; j < kRankTile; j += 256) keys[j] = j0 + j < M ? embed_key(tok, j0 + j, vocab) : INT_MAX;  // (above every key)
        __syncthreads();
        if (j0 + kRankTile <= m0)
            rank += count_below<0>(keys, j0, mine, m);
        else if (j0 >= m0 + 256)
            rank += count_below<2>(keys, j0, mine, m);
        else
            rank += count_below<1>(keys, j0, mine, m);
    }
    if (m < M) {
        order[rank] = m;
        sorted[rank] = mine;
    }
}

__global__ void __launch_bounds__(256) embed_word_grad_kernel(const float* __restrict__ grad, const int* __restrict__ order,
                                                              const int* __restrict__ sorted, int M, int vocab, int padding_idx,
                                                              float* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    for (int v = blockIdx.x * 4 + wave; v < vocab; v += gridDim.x * 4) {
        Row acc = splat(0.f);
        // the run of v: [lo, end) of sorted, empty for the padding row (its tokens are in the order, but the row takes none)
        int lo = 0, hi = M;
        if (v == padding_idx) lo = M;
        while (lo < hi) {       // the first i with sorted[i] >= v
            const int mid = (lo + hi) >> 1;
            if (sorted[mid] < v) lo = mid + 1; else hi = mid;
        }
        if (lo < M && sorted[lo] == v) {
            int end = lo + 1;
            hi = M;
            while (end < hi) {      // the first i > lo with sorted[i] > v
                const int mid = (end + hi) >> 1;
                if (sorted[mid] <= v) end = mid + 1; else hi = mid;
            }
            acc = load_row(grad + (size_t)order[lo] * kD, lane);       // the sum starts from the run's first row
            int i = lo + 1;
            for (; i + kRunLoads <= end; i += kRunLoads) {
                Row r[kRunLoads];
#pragma unroll
                for (int u = 0; u < kRunLoads; ++u) r[u] = load_row(grad + (size_t)order[i + u] * kD, lane);
#pragma unroll
                for (int u = 0; u < kRunLoads; ++u) add_row(acc, r[u]);
            }
            for (; i < end; ++i) add_row(acc, load_row(grad + (size_t)order[i] * kD, lane));
        }
        store_row(out + (size_t)v * kD, lane, acc);
    }
}

__global__ void __launch_bounds__(256) embed_pos_grad_kernel(const float* __restrict__ grad, int64_t B, int64_t L, int64_t max_pos,
                                                             float* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int64_t l = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (l >= max_pos) return;
    Row acc = splat(0.f);
    if (l < L) {
        const float* g = grad + l * kD;
        const size_t doc = (size_t)L * kD;
        acc = load_row(g, lane);
        int64_t b = 1;
        for (; b + 4 <= B; b += 4) {
            Row r[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) r[u] = load_row(g + (b + u) * doc, lane);
#pragma unroll
            for (int u = 0; u < 4; ++u) add_row(acc, r[u]);
        }
        for (; b < B; ++b) add_row(acc, load_row(g + b * doc, lane));
    }
    store_row(out + l * kD, lane, acc);
}

__global__ void __launch_bounds__(4 * kTypeParts) embed_type_grad_kernel(const float* __restrict__ grad, const int64_t* __restrict__ typ,
                                                                         int64_t M, float* __restrict__ out) {
    __shared__ v4 part[kTypeParts][kTypeCols / 4];
    const int q = threadIdx.x & 3, j = threadIdx.x >> 2;
    const int64_t t = blockIdx.y;
    const int col = blockIdx.x * kTypeCols + 4 * q;
    const int64_t R = (M + kTypeParts - 1) / kTypeParts;
    const int64_t r0 = j * R, r1 = r0 + R < M ? r0 + R : M;
    const v4 zero = {0.f, 0.f, 0.f, 0.f};
    v4 acc = zero;
    int64_t r = r0;
    for (; r + 4 <= r1; r += 4) {
        v4 x[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            x[u] = *reinterpret_cast<const v4*>(grad + (r + u) * kD + col);
            if ((typ ? typ[r + u] : 0) != t) x[u] = zero;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) acc += x[u];
    }
    for (; r < r1; ++r) {
        const v4 x = *reinterpret_cast<const v4*>(grad + r * kD + col);
        acc += (typ ? typ[r] : 0) == t ? x : zero;
    }
    part[j][q] = acc;
    __syncthreads();
    if (threadIdx.x < kTypeCols / 4) {
        v4 s = zero;
        for (int p = 0; p < kTypeParts; ++p) s += part[p][threadIdx.x];
        *reinterpret_cast<v4*>(out + t * kD + col) = s;
    }
}

size_t embed_ws_bytes(int64_t M) {
    const size_t raw = M > 0 ? 2 * (size_t)M * sizeof(int) : 0;      // order [M], sorted [M]
    return raw < 16 ? 16 : (raw + 15) & ~(size_t)15;
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

int embed_shape_check(const char* who, int64_t B, int64_t L, int64_t vocab, int64_t max_pos, int64_t n_types) {
    ASPIRE_REQUIRE(vocab > 0, ASPIRE_ERR_INVALID_ARG, "%s: vocab = %lld must be positive", who, (long long)vocab);
    ASPIRE_REQUIRE(max_pos > 0, ASPIRE_ERR_INVALID_ARG, "%s: max_pos = %lld must be positive", who, (long long)max_pos);
    ASPIRE_REQUIRE(n_types > 0, ASPIRE_ERR_INVALID_ARG, "%s: n_types = %lld must be positive", who, (long long)n_types);
    ASPIRE_REQUIRE(B >= 0, ASPIRE_ERR_INVALID_ARG, "%s: B = %lld is negative", who, (long long)B);
    ASPIRE_REQUIRE(L > 0 && L <= max_pos, ASPIRE_ERR_INVALID_ARG, "%s: L = %lld outside (0, max_pos = %lld]", who, (long long)L,
                   (long long)max_pos);
    ASPIRE_REQUIRE(vocab < INT_MAX && max_pos < INT_MAX && n_types < INT_MAX, ASPIRE_ERR_UNSUPPORTED,
                   "%s: a table of 2^31 - 1 rows or more (vocab = %lld, max_pos = %lld, n_types = %lld)", who, (long long)vocab,
                   (long long)max_pos, (long long)n_types);
    ASPIRE_REQUIRE(B <= (INT64_MAX / kD) / L, ASPIRE_ERR_UNSUPPORTED, "%s: B * L * 768 overflows (B = %lld, L = %lld)", who, (long long)B,
                   (long long)L);
    return ASPIRE_OK;
}

}  // namespace
}  // namespace aspire

using namespace aspire;

extern "C" int aspire_bert_embed_sum_f32(const float* word, const float* pos, const float* type, const int64_t* tok, const int64_t* typ,
                                         int64_t B, int64_t L, int64_t vocab, int64_t max_pos, int64_t n_types, float* out, void* stream) {
    const char* who = "aspire_bert_embed_sum_f32";
    ASPIRE_REQUIRE(word && pos && type, ASPIRE_ERR_INVALID_ARG, "%s: null table (word %p, pos %p, type %p)", who, (const void*)word,
                   (const void*)pos, (const void*)type);
    ASPIRE_REQUIRE(tok, ASPIRE_ERR_INVALID_ARG, "%s: null tok", who);
    ASPIRE_REQUIRE(out, ASPIRE_ERR_INVALID_ARG, "%s: null out", who);
    if (const int rc = embed_shape_check(who, B, L, vocab, max_pos, n_types)) return rc;
    ASPIRE_REQUIRE(aligned16(word) && aligned16(pos) && aligned16(type) && aligned16(out), ASPIRE_ERR_INVALID_ARG,
                   "%s: a table or out is not 16-byte aligned (word %p, pos %p, type %p, out %p)", who, (const void*)word, (const void*)pos,
                   (const void*)type, (const void*)out);
    if (B == 0) return ASPIRE_OK;
    const int64_t rows = B * L;
    ASPIRE_REQUIRE((rows + 3) / 4 <= INT_MAX, ASPIRE_ERR_UNSUPPORTED, "%s: %lld token rows are beyond one launch", who, (long long)rows);
    hipLaunchKernelGGL(embed_sum_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, static_cast<hipStream_t>(stream), word, pos, type,
                       tok, typ, rows, L, vocab, n_types, out);
    ASPIRE_LAUNCH_OK();
    return ASPIRE_OK;
}

extern "C" size_t aspire_bert_embed_workspace_bytes(int64_t M, int64_t vocab) {
    (void)vocab;        // the sorted order is per token row; the table's height does not enter
    return embed_ws_bytes(M);
}

extern "C" int aspire_bert_embed_backward_f32(const float* grad_emb_sum, const int64_t* tok, const int64_t* typ, int64_t B, int64_t L,
                                              int64_t vocab, int64_t max_pos, int64_t n_types, int64_t padding_idx, float* grad_word,
                                              float* grad_pos, float* grad_type, void* ws, size_t ws_bytes, void* stream) {
    const char* who = "aspire_bert_embed_backward_f32";
    if (const int rc = embed_shape_check(who, B, L, vocab, max_pos, n_types)) return rc;
    ASPIRE_REQUIRE(padding_idx >= -1 && padding_idx < vocab, ASPIRE_ERR_INVALID_ARG, "%s: padding_idx = %lld outside [-1, vocab = %lld)",
                   who, (long long)padding_idx, (long long)vocab);
    if (!grad_word && !grad_pos && !grad_type) return ASPIRE_OK;
    ASPIRE_REQUIRE(grad_emb_sum, ASPIRE_ERR_INVALID_ARG, "%s: null grad_emb_sum with a table's gradient wanted", who);
    ASPIRE_REQUIRE(aligned16(grad_emb_sum) && aligned16(grad_word) && aligned16(grad_pos) && aligned16(grad_type), ASPIRE_ERR_INVALID_ARG,
                   "%s: a gradient is not 16-byte aligned (grad_emb_sum %p, grad_word %p, grad_pos %p, grad_type %p)", who,
                   (const void*)grad_emb_sum, (const void*)grad_word, (const void*)grad_pos, (const void*)grad_type);
    const int64_t M = B * L;
    if (grad_word) {
        ASPIRE_REQUIRE(tok, ASPIRE_ERR_INVALID_ARG, "%s: null tok with grad_word wanted", who);
        ASPIRE_REQUIRE(M <= kEmbedMaxRows, ASPIRE_ERR_UNSUPPORTED, "%s: %lld token rows, the rank pass serves %lld", who, (long long)M,
                       (long long)kEmbedMaxRows);
        const size_t need = embed_ws_bytes(M);
        ASPIRE_REQUIRE(ws, ASPIRE_ERR_INVALID_ARG, "%s: null workspace (aspire_bert_embed_workspace_bytes(%lld, %lld) = %zu)", who,
                       (long long)M, (long long)vocab, need);
        ASPIRE_REQUIRE(ws_bytes >= need, ASPIRE_ERR_INVALID_ARG, "%s: workspace of %zu bytes is too small, need %zu", who, ws_bytes, need);
        ASPIRE_REQUIRE(aligned16(ws), ASPIRE_ERR_INVALID_ARG, "%s: workspace %p is not 16-byte aligned", who, ws);
    }
    ASPIRE_REQUIRE(!grad_type || n_types <= 65535, ASPIRE_ERR_UNSUPPORTED, "%s: n_types = %lld beyond one launch's 65535", who,
                   (long long)n_types);
    if (B == 0) return ASPIRE_OK;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (grad_word) {
        int* order = static_cast<int*>(ws);
        int* sorted = order + M;
        hipLaunchKernelGGL(embed_rank_kernel, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, st, tok, (int)M, (int)vocab, order, sorted);
        ASPIRE_LAUNCH_OK();
        const int64_t groups = (vocab + 3) / 4;
        hipLaunchKernelGGL(embed_word_grad_kernel, dim3((unsigned)(groups < kMaxGrid ? groups : kMaxGrid)), dim3(256), 0, st, grad_emb_sum,
                           order, sorted, (int)M, (int)vocab, (int)padding_idx, grad_word);
        ASPIRE_LAUNCH_OK();
    }
    if (grad_pos) {
        hipLaunchKernelGGL(embed_pos_grad_kernel, dim3((unsigned)((max_pos + 3) / 4)), dim3(256), 0, st, grad_emb_sum, B, L, max_pos, grad_pos);
        ASPIRE_LAUNCH_OK();
    }
    if (grad_type) {
        hipLaunchKernelGGL(embed_type_grad_kernel, dim3(kD / kTypeCols, (unsigned)n_types), dim3(4 * kTypeParts), 0, st, grad_emb_sum, typ, M,
                           grad_type);
        ASPIRE_LAUNCH_OK();
    }
    return ASPIRE_OK;
}
