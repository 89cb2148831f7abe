// The encoder's attention kernels.  The forward's plan (encoder.hip: plan_forward, run_layer) decides which form runs.
//
// Kernels
//   flash_attn_p_kernel      fused attention for one (document, head, 128 queries) on the fp16 planes the QKV GEMM writes (gemm_p_qkv_kernel),
//                            K / V tiles by LDS-DMA: the default on the plane path
//   flash_attn_p64_kernel    the same on 64-key tiles, three workgroups per CU (ASPIRE_HIP_ATTN=p64)
//   flash_attn_f16x2_kernel  fused attention on fp32 Q / K / V, split into fp16 planes inside the kernel: the default without the QKV planes
//                            (below 1024 token rows, ASPIRE_HIP_ATTN=f16x2, pinned GEMM tiles)
//   flash_attn_f32_kernel    fused attention on fp32-input MFMAs (round 2; ASPIRE_HIP_ATTN=f32)
//   softmax_mask_kernel      rows of scores: x*scale + key-padding bias, softmax in place (one wave per row); between the two batched GEMMs
//                            of the three-kernel form (ASPIRE_HIP_ATTN=gemm) that the fused kernels are tested against
//   cls_attn_kernel          attention of the CLS query alone, one workgroup per (document, head) (aspire_bert_forward_cls_f32's last layer)
//
// BIAS (template parameter of every kernel but flash_attn_p64_kernel and cls_attn_kernel): MPNet's relative-position bias
// (aspire_bert_extras::rel_bias: HF MPNetSelfAttention, q.k / 8, + position_bias, + mask, soft-max).  rel_bias is
// [heads][2 rel_span - 1], entry (j - i) + rel_span - 1 the bias of (query i, key j); it is the same in every layer.  BIAS = false is
// BertModel's attention: the instantiations the BERT forwards run contain nothing of the bias (if constexpr).
// The fused kernels keep the head's table in LDS (stage_rel_bias: 4 KB, the 2 L - 1 <= 1023 distances of this document length,
// already times log2(e) as their exp2 soft-max wants the scores): a lane reads 16 n entries per n-key tile, at addresses that differ
// by (key - query) only -- consecutive words across the lanes of a wave, no bank conflict -- and LDS reads count on lgkmcnt, apart from
// the vmcnt that flash_attn_p_kernel's LDS-DMA waits on.  66 + 4 KB still fits twice per CU.
#include <math.h>

#include "enc_planes.h"
#include "enc_types.h"

namespace aspire {
namespace {

// scores [rows = B*H*L][ld] in place: softmax_j(x_j * scale + (mask[b][j] ? 0 : -FLT_MAX)); columns in [L, ld)
// are written as zeros so that the P.V GEMM can run K up to ld.
// BIAS: + rel_bias[h][(j - i) + rel_span - 1] between the scaling and the mask (row = (b H + h) L + i)
template <bool BIAS>
__global__ void __launch_bounds__(256) softmax_mask_kernel(float* __restrict__ s, const int64_t* __restrict__ mask, int64_t rows,
                                                           int L, int ld, int rows_per_doc, float scale,
                                                           const float* __restrict__ rel_bias, int rel_span) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int64_t b = row / rows_per_doc;
    float* p = s + row * ld;
    const int64_t* mk = mask + b * L;
    constexpr int kMaxPer = 8;  // L <= 512
    float v[kMaxPer];
    float m = -INFINITY;
    const float* rb = nullptr;   // BIAS: this row's bias of key j at rb[j]
    if constexpr (BIAS) {
        const int i = (int)(row % L), h = (int)((row % rows_per_doc) / L);
        rb = rel_bias + (size_t)h * (2 * rel_span - 1) + (rel_span - 1 - i);
    }
#pragma unroll
    for (int c = 0; c < kMaxPer; ++c) {
        const int j = lane + 64 * c;
        if (j < L) {
            // (1 - mask) * finfo(float32).min added to the scaled scores, as BertModel's extended mask
            if constexpr (BIAS)
                v[c] = (p[j] * scale + rb[j]) + (mk[j] != 0 ? 0.f : -3.4028234663852886e38f);
            else
                v[c] = p[j] * scale + (mk[j] != 0 ? 0.f : -3.4028234663852886e38f);
            m = fmaxf(m, v[c]);
        } else {
            v[c] = -INFINITY;
        }
    }
    m = wave_max(m);
    float sum = 0.f;
#pragma unroll
    for (int c = 0; c < kMaxPer; ++c) {
        v[c] = (lane + 64 * c < L) ? expf(v[c] - m) : 0.f;
        sum += v[c];
    }
    const float inv = 1.0f / wave_sum(sum);
#pragma unroll
    for (int c = 0; c < kMaxPer; ++c) {
        const int j = lane + 64 * c;
        if (j < ld) p[j] = v[c] * inv;
    }
}

// ---------------------------------------------------------------------------------------------------------------
// Fused attention for one (document, head, 128 queries): softmax(Q K^T / 8 + mask) V without the [L, L] score
// matrix ever leaving the chip (the three-kernel form writes it, reads and rewrites it in the softmax, and reads it
// again: 400 MB per layer at B = 32, L = 256).  Everything is computed TRANSPOSED so that probabilities never change
// layout between the two products:
//   S^T = K Q^T   : keys are the MFMA M side, queries the N side -> in the 32x32 C layout lane n = lane & 31 is a
//                   QUERY and its 16 accumulator registers (x 4 row blocks) are KEYS.  The soft-max over keys is
//                   therefore in-register per lane, plus ONE exchange with lane ^ 32 (the other half of the keys).
//   O^T = V^T P^T : P^T is the B operand [k = key][n = query] -- lane n = query again, and the MFMA's k pair is
//                   (lanes < 32, lanes >= 32) = exactly the two key halves the C layout left in those lanes.  So
//                   accumulator register t of S^T goes straight back in as the B operand of step t.
// A wave owns 32 queries (their Q rows live in 32 registers for the whole kernel) and all keys; the 4 waves of a
// workgroup share the K tile (staged k-major, dims paired (d, d+8) so the half-waves read opposite LDS bank
// halves) and the V tile (row-major, 72-float rows: keys 4 apart land 32 banks apart).  Keys are walked in
// tiles of 128 with the usual running max / sum rescaling (flash attention), all in fp32 with exp2.
// HF semantics kept: scores / sqrt(64) + (1 - mask) * finfo.min, soft-max over keys (modeling_bert.py), for any 0/1 mask (key_bias_log2).
// ---------------------------------------------------------------------------------------------------------------
constexpr int kFaLdK = 132, kFaLdV = 72;
// The fused kernels' bias table (BIAS): tab[t] = log2(e) x the bias of distance (key - query) = t - (L - 1) of head h, zero beyond
// the 2 L - 1 distances of this length (a tile's padding keys and a block's padding queries read there; their scores are masked or
// never stored, but must stay finite).  Query i, key j: tab[j - min(i, L - 1) + L - 1], j <= 511: an index in [0, 1022].
constexpr int kRelTab = 1024;
__device__ __forceinline__ void stage_rel_bias(float* tab, const float* __restrict__ rel_bias, int rel_span, int h, int L, int tid) {
    const float* rb = rel_bias + (size_t)h * (2 * rel_span - 1) + (rel_span - L);
    for (int t = tid; t < kRelTab; t += 256) tab[t] = t < 2 * L - 1 ? rb[t] * 1.44269504088896340736f : 0.f;
}
// The fused kernels' additive key mask, in the log2 units of their exp2 soft-max.  A masked key gets -FLT_MAX, FINITE, as softmax_mask_kernel
// and cls_attn_kernel keep it and as HF's (1 - mask) * finfo.min is: a score plus it rounds to -FLT_MAX itself, so next to one real key a
// masked key weighs exp2(-FLT_MAX - max) = 0, a key tile without a real key leaves a finite running max that the first real key
// flushes (alpha = exp2(-FLT_MAX - max) = 0), and a row without any real key attends uniformly over its L keys.  (Times log2(e) the
// constant would overflow to -inf, and a first tile of -inf alone makes alpha = exp2(-inf + inf) = NaN for good.)  Keys past L are tile
// padding -- other documents' rows -- and weigh exactly 0 in every case: -inf, which a tile never holds alone.
__device__ __forceinline__ float key_bias_log2(const int64_t* __restrict__ mask_row, int kk, int L) {
    return kk >= L ? -INFINITY : (mask_row[kk] != 0 ? 0.f : -3.4028234663852886e38f);
}
// ctxp (optional, instead of ctx): the context rows go out in the P layout [rows, 768] -- the A operand of the output projection
template <bool BIAS>
__global__ void __launch_bounds__(256, 2) flash_attn_f32_kernel(const float* __restrict__ qkv, const int64_t* __restrict__ mask,
                                                                float* __restrict__ ctx, int L, int H, void* __restrict__ ctxp,
                                                                int64_t rows, const float* __restrict__ rel_bias, int rel_span) {
    __shared__ __attribute__((aligned(16))) float Ks[64][kFaLdK];     // [dim][key]
    __shared__ __attribute__((aligned(16))) float Vs[128][kFaLdV];    // [key][dim]
    __shared__ float kbias[128];
    __shared__ float rtab[BIAS ? kRelTab : 1];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lr = lane & 31, lk = lane >> 5;
    const int qblocks = (L + 127) / 128;
    const int qb = blockIdx.x % qblocks, h = (blockIdx.x / qblocks) % H, b = blockIdx.x / (qblocks * H);
    const size_t ld = 3 * kD;
    const float* base = qkv + (size_t)b * L * ld + h * 64;
    const int q_row = qb * 128 + wave * 32 + lr;                      // this lane's query
    const bool q_ok = q_row < L;
    const float* rq = nullptr;                                         // BIAS: this lane's bias of key j (log2 units) at rq[j]
    if constexpr (BIAS) {
        stage_rel_bias(rtab, rel_bias, rel_span, h, L, tid);           // (read behind the key loop's barriers)
        rq = rtab + (L - 1 - min(q_row, L - 1));
    }
    // Q^T operand registers: step t = 8 G + j multiplies dims (16 G + j | 16 G + 8 + j) in lanes (< 32 | >= 32)
    float qreg[32];
    {
        const float* qp = base + (size_t)min(q_row, L - 1) * ld;
#pragma unroll
        for (int G = 0; G < 4; ++G) {
            const float4 u = *reinterpret_cast<const float4*>(qp + 16 * G + 8 * lk);
            const float4 v = *reinterpret_cast<const float4*>(qp + 16 * G + 8 * lk + 4);
            qreg[8 * G + 0] = u.x; qreg[8 * G + 1] = u.y; qreg[8 * G + 2] = u.z; qreg[8 * G + 3] = u.w;
            qreg[8 * G + 4] = v.x; qreg[8 * G + 5] = v.y; qreg[8 * G + 6] = v.z; qreg[8 * G + 7] = v.w;
        }
    }
    f32x16 o[2];
#pragma unroll
    for (int mb = 0; mb < 2; ++mb)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[mb][r] = 0.f;
    float m_run = -INFINITY, l_run = 0.f;                              // l_run: this half-wave's share of the sum
    constexpr float kScaleLog2 = 0.125f * 1.44269504088896340736f;     // 1/sqrt(64) folded with log2(e)

    for (int k0 = 0; k0 < L; k0 += 128) {
        __syncthreads();                                               // previous tile fully consumed
        // ---- stage K (transposed) and V: thread -> key tid >> 1, 32 dims (tid & 1) * 32 .. -------------------
        {
            const int key = tid >> 1, d0 = (tid & 1) * 32;
            const bool ok = k0 + key < L;
            const float* kp = base + kD + (size_t)min(k0 + key, L - 1) * ld + d0;
            const float* vp = kp + kD;
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                float4 kv = *reinterpret_cast<const float4*>(kp + 4 * c);
                float4 vv = *reinterpret_cast<const float4*>(vp + 4 * c);
                if (!ok) kv = vv = make_float4(0.f, 0.f, 0.f, 0.f);
                Ks[d0 + 4 * c + 0][key] = kv.x;
                Ks[d0 + 4 * c + 1][key] = kv.y;
                Ks[d0 + 4 * c + 2][key] = kv.z;
                Ks[d0 + 4 * c + 3][key] = kv.w;
                *reinterpret_cast<float4*>(&Vs[key][d0 + 4 * c]) = vv;
            }
            if (tid < 128) {
                const int kk = k0 + tid;
                kbias[tid] = key_bias_log2(mask + (size_t)b * L, kk, L);
            }
        }
        __syncthreads();
        // ---- S^T tile: 4 blocks of 32 keys x this wave's 32 queries -------------------------------------------
        f32x16 sacc[4];
#pragma unroll
        for (int rb = 0; rb < 4; ++rb)
#pragma unroll
            for (int r = 0; r < 16; ++r) sacc[rb][r] = 0.f;
#pragma unroll
        for (int t = 0; t < 32; ++t) {
            const int d = 16 * (t >> 3) + (t & 7) + 8 * lk;
#pragma unroll
            for (int rb = 0; rb < 4; ++rb)
                sacc[rb] = __builtin_amdgcn_mfma_f32_32x32x2f32(Ks[d][32 * rb + lr], qreg[t], sacc[rb], 0, 0, 0);
        }
        // ---- online soft-max over this tile's keys (registers of this lane + the other half-wave) -------------
        float tmax = -INFINITY;
#pragma unroll
        for (int rb = 0; rb < 4; ++rb)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int key = 32 * rb + 8 * (r >> 2) + 4 * lk + (r & 3);
                // scores * (1/8) in log2 units + mask (key_bias_log2)
                if constexpr (BIAS)
                    sacc[rb][r] = fmaf(sacc[rb][r], kScaleLog2, rq[k0 + key]) + kbias[key];
                else
                    sacc[rb][r] = fmaf(sacc[rb][r], kScaleLog2, kbias[key]);
                tmax = fmaxf(tmax, sacc[rb][r]);
            }
        tmax = fmaxf(tmax, lane_xor<32>(tmax));
        const float m_new = fmaxf(m_run, tmax);
        const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);     // exp2(-inf) = 0 on the first tile
        float psum = 0.f;
#pragma unroll
        for (int rb = 0; rb < 4; ++rb)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                sacc[rb][r] = __builtin_amdgcn_exp2f(sacc[rb][r] - m_new);
                psum += sacc[rb][r];
            }
        l_run = fmaf(l_run, alpha, psum);
        m_run = m_new;
#pragma unroll
        for (int mb = 0; mb < 2; ++mb)
#pragma unroll
            for (int r = 0; r < 16; ++r) o[mb][r] *= alpha;
        // ---- O^T += V^T P^T: accumulator register t of S^T is the B operand of step t -------------------------
#pragma unroll
        for (int rb = 0; rb < 4; ++rb)
#pragma unroll
            for (int t = 0; t < 16; ++t) {
                const int key = 32 * rb + 8 * (t >> 2) + 4 * lk + (t & 3);
#pragma unroll
                for (int mb = 0; mb < 2; ++mb)
                    o[mb] = __builtin_amdgcn_mfma_f32_32x32x2f32(Vs[key][32 * mb + lr], sacc[rb][t], o[mb], 0, 0, 0);
            }
    }
    // ---- normalise and store: lane = query, registers = head dims (4 consecutive per group) --------------------
    const float l_tot = l_run + lane_xor<32>(l_run);
    const float inv = 1.0f / l_tot;
    if (q_ok && ctxp) {
#pragma unroll
        for (int mb = 0; mb < 2; ++mb)
#pragma unroll
            for (int g4 = 0; g4 < 4; ++g4)
                p_store4(ctxp, rows, (int64_t)b * L + q_row, h * 64 + 32 * mb + 8 * g4 + 4 * lk, o[mb][4 * g4 + 0] * inv,
                         o[mb][4 * g4 + 1] * inv, o[mb][4 * g4 + 2] * inv, o[mb][4 * g4 + 3] * inv);
    } else if (q_ok) {
        float* op = ctx + ((size_t)b * L + q_row) * kD + h * 64;
#pragma unroll
        for (int mb = 0; mb < 2; ++mb)
#pragma unroll
            for (int g4 = 0; g4 < 4; ++g4)
                *reinterpret_cast<float4*>(op + 32 * mb + 8 * g4 + 4 * lk) =
                    make_float4(o[mb][4 * g4 + 0] * inv, o[mb][4 * g4 + 1] * inv, o[mb][4 * g4 + 2] * inv, o[mb][4 * g4 + 3] * inv);
    }
}

// ---------------------------------------------------------------------------------------------------------------
// The same fused attention on the fp16 matrix pipe at fp32 accuracy: every operand (Q, K, V, and the probabilities)
// goes in as two fp16 planes h + l (module comment of the P-layout GEMM: 24 significant bits; Q / K / V are O(1), P is in
// [0, 1]), three v_mfma_f32_32x32x16_f16 per term, sums and the whole soft-max in fp32.  Per 128-key tile and wave that is
// 96 MFMAs of 32 cycles against 256 fp32-input MFMAs of 64: 3 072 matrix-pipe cycles instead of 16 384.
//   S^T = K Q^T  : A = K planes [key][64 dims] (128-byte rows, 16-byte pieces XORed with the key's bits 1..3: conflict-free
//                  ds_read_b128), B = this lane's query, split once into 4 k steps x (h, l) registers.
//   O^T = V^T P^T: the MFMA's 8 consecutive k of lane half lk must be KEYS.  The S^T accumulators of lane half lk hold, per
//                  16-key group, keys {4 lk .. 4 lk + 3} and {8 + 4 lk .. 8 + 4 lk + 3}: P^T goes back in straight from the
//                  registers (converted to h + l in place), and the V^T image is built to match -- [dim][key slot], slots of a
//                  16-key group ordered [0-3, 8-11, 4-7, 12-15], so that a lane's 8 keys are one 16-byte read (256-byte rows,
//                  pieces XORed with the dim's low 4 bits).  V is transposed while it is staged: a thread owns 4 consecutive
//                  keys x 8 dims and writes 8-byte runs of 4 keys.
// ---------------------------------------------------------------------------------------------------------------
template <bool BIAS>
__global__ void __launch_bounds__(256, 2) flash_attn_f16x2_kernel(const float* __restrict__ qkv, const int64_t* __restrict__ mask,
                                                                  float* __restrict__ ctx, int L, int H, void* __restrict__ ctxp,
                                                                  int64_t rows, const float* __restrict__ rel_bias, int rel_span) {
    __shared__ __attribute__((aligned(16))) unsigned char Kp[2][128 * 128];    // [plane][key][64 dims fp16]
    __shared__ __attribute__((aligned(16))) unsigned char Vp[2][64 * 256];     // [plane][dim][128 key slots fp16]
    __shared__ float kbias[128];
    __shared__ float rtab[BIAS ? kRelTab : 1];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lr = lane & 31, lk = lane >> 5;
    const int qblocks = (L + 127) / 128;
    // XCD-aware order (as the GEMMs'): XCD x = workgroup id mod 8 takes a contiguous run of the (document, head, query block) sequence, so the
    // query blocks of one (document, head) -- which stage the same K and V -- share an L2
    uint32_t wl;
    {
        const uint32_t nb = gridDim.x, bid = blockIdx.x, x = bid & 7, q8 = nb >> 3, r8 = nb & 7;
        wl = x * q8 + (x < r8 ? x : r8) + (bid >> 3);
    }
    const int qb = wl % qblocks, h = (wl / qblocks) % H, b = wl / (qblocks * H);
    const size_t ld = 3 * kD;
    const float* base = qkv + (size_t)b * L * ld + h * 64;
    const int q_row = qb * 128 + wave * 32 + lr;                      // this lane's query
    const bool q_ok = q_row < L;
    const float* rq = nullptr;                                         // BIAS: this lane's bias of key j (log2 units) at rq[j]
    if constexpr (BIAS) {
        stage_rel_bias(rtab, rel_bias, rel_span, h, L, tid);           // (read behind the key loop's barriers)
        rq = rtab + (L - 1 - min(q_row, L - 1));
    }
    f16x8_t qh[4], ql[4];                                              // k step ks: dims 16 ks + 8 lk .. + 7
    {
        const float* qp = base + (size_t)min(q_row, L - 1) * ld + 8 * lk;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            const float4 u = *reinterpret_cast<const float4*>(qp + 16 * ks), v = *reinterpret_cast<const float4*>(qp + 16 * ks + 4);
            const float x[8] = {u.x, u.y, u.z, u.w, v.x, v.y, v.z, v.w};
            split8_f16(x, qh[ks], ql[ks]);
        }
    }
    f32x16 o[2];
#pragma unroll
    for (int mb = 0; mb < 2; ++mb)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[mb][r] = 0.f;
    float m_run = -INFINITY, l_run = 0.f;                              // l_run: this half-wave's share of the sum
    constexpr float kScaleLog2 = 0.125f * 1.44269504088896340736f;     // 1/sqrt(64) folded with log2(e)
    // fragment addresses: K rows 32 rb + lr, piece (2 ks + lk) ^ ((row >> 1) & 7); V^T rows 32 mb + lr, piece (2 s16 + lk) ^ (row & 15)
    const uint32_t k_rd = lr * 128 + 16 * (lk ^ ((lr >> 1) & 7)), k_sw = 0;
    (void)k_sw;
    const uint32_t v_rd = lr * 256 + 16 * (lk ^ (lr & 15) ^ (2 * (lr >> 4)));      // piece ^ f(row), f(d) = (d & 15) ^ 2 (d >> 4): see the V^T store

    for (int k0 = 0; k0 < L; k0 += 128) {
        __syncthreads();                                               // previous tile fully consumed
        {
            // ---- K: thread -> key tid >> 1, 32 dims (tid & 1) * 32 ..: four 8-dim pieces per plane ----
            const int key = tid >> 1, d0 = (tid & 1) * 32;
            const bool ok = k0 + key < L;
            const float* kp = base + kD + (size_t)min(k0 + key, L - 1) * ld + d0;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                float4 u = *reinterpret_cast<const float4*>(kp + 8 * c), v = *reinterpret_cast<const float4*>(kp + 8 * c + 4);
                if (!ok) u = v = make_float4(0.f, 0.f, 0.f, 0.f);
                const float x[8] = {u.x, u.y, u.z, u.w, v.x, v.y, v.z, v.w};
                f16x8_t hh, ll;
                split8_f16(x, hh, ll);
                const uint32_t at = key * 128 + 16 * ((d0 / 8 + c) ^ ((key >> 1) & 7));
                *reinterpret_cast<f16x8_t*>(&Kp[0][at]) = hh;
                *reinterpret_cast<f16x8_t*>(&Kp[1][at]) = ll;
            }
            // ---- V transposed: thread -> keys 4 kg .. 4 kg + 3 (kg = tid >> 3), dims 8 dg .. 8 dg + 7 (dg = tid & 7) ----
            const int kg = tid >> 3, dg = tid & 7;
            float vv[4][8];
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) {
                const int vkey = k0 + 4 * kg + kk;
                const float* vp = base + 2 * kD + (size_t)min(vkey, L - 1) * ld + 8 * dg;
                float4 u = *reinterpret_cast<const float4*>(vp), v = *reinterpret_cast<const float4*>(vp + 4);
                if (vkey >= L) u = v = make_float4(0.f, 0.f, 0.f, 0.f);
                vv[kk][0] = u.x; vv[kk][1] = u.y; vv[kk][2] = u.z; vv[kk][3] = u.w;
                vv[kk][4] = v.x; vv[kk][5] = v.y; vv[kk][6] = v.z; vv[kk][7] = v.w;
            }
            const int sub = kg & 3, slot4 = sub == 1 ? 2 : sub == 2 ? 1 : sub;      // [0-3, 8-11, 4-7, 12-15] within a 16-key group
            const int piece = 2 * (kg >> 2) + (slot4 >> 1), half = slot4 & 1;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int d = 8 * dg + j;
                typedef _Float16 f16x4_t __attribute__((ext_vector_type(4)));
                f16x4_t hh, ll;
#pragma unroll
                for (int kk = 0; kk < 4; ++kk) {
                    const _Float16 t = (_Float16)vv[kk][j];
                    hh[kk] = t;
                    ll[kk] = (_Float16)(vv[kk][j] - (float)t);
                }
                // the 16-byte piece XORed with f(d) = (d & 15) ^ 2 (d >> 4): the rows are 256 B = all 64 banks apart, and a wave's
                // stores of one j go to rows d = 8 dg + j, dg = 0 .. 7 -- with d & 15 alone (round 3) only two different swizzles for
                // eight rows: every store was a 4-way bank conflict (round-5 counters: 3.1 M conflict cycles of 5.9 M LDS cycles)
                const uint32_t at = d * 256 + 16 * (piece ^ (d & 15) ^ (2 * (d >> 4))) + 8 * half;
                *reinterpret_cast<f16x4_t*>(&Vp[0][at]) = hh;
                *reinterpret_cast<f16x4_t*>(&Vp[1][at]) = ll;
            }
            if (tid < 128) {
                const int kk = k0 + tid;
                kbias[tid] = key_bias_log2(mask + (size_t)b * L, kk, L);
            }
        }
        __syncthreads();
        // ---- S^T tile: 4 blocks of 32 keys x this wave's 32 queries; per k step the products l.h, h.l, h.h ----
        f32x16 sacc[4];
#pragma unroll
        for (int rb = 0; rb < 4; ++rb)
#pragma unroll
            for (int r = 0; r < 16; ++r) sacc[rb][r] = 0.f;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks)
#pragma unroll
            for (int rb = 0; rb < 4; ++rb) {
                const uint32_t at = (k_rd + rb * 32 * 128) ^ (32 * ks);
                const f16x8_t kh = *reinterpret_cast<const f16x8_t*>(&Kp[0][at]), kl = *reinterpret_cast<const f16x8_t*>(&Kp[1][at]);
                sacc[rb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(kl, qh[ks], sacc[rb], 0, 0, 0);
                sacc[rb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(kh, ql[ks], sacc[rb], 0, 0, 0);
                sacc[rb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(kh, qh[ks], sacc[rb], 0, 0, 0);
            }
        // ---- online soft-max over this tile's keys (registers of this lane + the other half-wave) -------------
        float tmax = -INFINITY;
#pragma unroll
        for (int rb = 0; rb < 4; ++rb) {
            // (BIAS: a compiler fence per key block keeps the table reads 16 at a time: hoisted together, all 64 of a tile cost two
            // registers more than the 256 this kernel has)
            if constexpr (BIAS) asm volatile("" ::: "memory");
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int key = 32 * rb + 8 * (r >> 2) + 4 * lk + (r & 3);
                if constexpr (BIAS)
                    sacc[rb][r] = fmaf(sacc[rb][r], kScaleLog2, rq[k0 + key]) + kbias[key];
                else
                    sacc[rb][r] = fmaf(sacc[rb][r], kScaleLog2, kbias[key]);
                tmax = fmaxf(tmax, sacc[rb][r]);
            }
        }
        tmax = fmaxf(tmax, lane_xor<32>(tmax));
        const float m_new = fmaxf(m_run, tmax);
        const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);     // exp2(-inf) = 0 on the first tile
        float psum = 0.f;
#pragma unroll
        for (int rb = 0; rb < 4; ++rb)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                sacc[rb][r] = __builtin_amdgcn_exp2f(sacc[rb][r] - m_new);
                psum += sacc[rb][r];
            }
        l_run = fmaf(l_run, alpha, psum);
        m_run = m_new;
#pragma unroll
        for (int mb = 0; mb < 2; ++mb)
#pragma unroll
            for (int r = 0; r < 16; ++r) o[mb][r] *= alpha;
        // ---- O^T += V^T P^T: registers 8 g .. 8 g + 7 of S^T block rb are the 8 keys of k step 2 rb + g in this lane half ----
#pragma unroll
        for (int rb = 0; rb < 4; ++rb)
#pragma unroll
            for (int g2 = 0; g2 < 2; ++g2) {
                const float pv[8] = {sacc[rb][8 * g2 + 0], sacc[rb][8 * g2 + 1], sacc[rb][8 * g2 + 2], sacc[rb][8 * g2 + 3],
                                     sacc[rb][8 * g2 + 4], sacc[rb][8 * g2 + 5], sacc[rb][8 * g2 + 6], sacc[rb][8 * g2 + 7]};
                f16x8_t ph, pl;
                split8_f16(pv, ph, pl);
                const int s16 = 2 * rb + g2;
#pragma unroll
                for (int mb = 0; mb < 2; ++mb) {
                    const uint32_t at = (v_rd + mb * 32 * 256) ^ (32 * s16) ^ (64 * mb);      // (row >> 4 = 2 mb + (lr >> 4))
                    const f16x8_t vh = *reinterpret_cast<const f16x8_t*>(&Vp[0][at]), vl = *reinterpret_cast<const f16x8_t*>(&Vp[1][at]);
                    o[mb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vl, ph, o[mb], 0, 0, 0);
                    o[mb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vh, pl, o[mb], 0, 0, 0);
                    o[mb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vh, ph, o[mb], 0, 0, 0);
                }
            }
    }
    // ---- normalise and store: lane = query, registers = head dims (4 consecutive per group) --------------------
    const float l_tot = l_run + lane_xor<32>(l_run);
    const float inv = 1.0f / l_tot;
    if (ctxp) {
        // the lane pair exchanges register groups (v_permlane32_swap, as the GEMM epilogues do): a lane owns dims 16 t + 8 lk .. + 7 of a
        // 32-dim block = one whole 16-byte piece per plane (8-byte stores before)
#pragma unroll
        for (int mb = 0; mb < 2; ++mb)
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                float x[8];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float fa = o[mb][8 * t + e] * inv, fb = o[mb][8 * t + 4 + e] * inv;
                    auto r = __builtin_amdgcn_permlane32_swap(__builtin_bit_cast(int, fa), __builtin_bit_cast(int, fb), false, false);
                    const int x0 = r[0], x1 = r[1];
                    x[e] = __builtin_bit_cast(float, x0);
                    x[4 + e] = __builtin_bit_cast(float, x1);
                }
                if (q_ok) p_store8_at(ctxp, p_slot8((uint32_t)rows, (uint32_t)(b * L + q_row), (uint32_t)(h * 64 + 32 * mb + 16 * t + 8 * lk)), x);
            }
    } else if (q_ok) {
        float* op = ctx + ((size_t)b * L + q_row) * kD + h * 64;
#pragma unroll
        for (int mb = 0; mb < 2; ++mb)
#pragma unroll
            for (int g4 = 0; g4 < 4; ++g4)
                *reinterpret_cast<float4*>(op + 32 * mb + 8 * g4 + 4 * lk) =
                    make_float4(o[mb][4 * g4 + 0] * inv, o[mb][4 * g4 + 1] * inv, o[mb][4 * g4 + 2] * inv, o[mb][4 * g4 + 3] * inv);
    }
}

// ---------------------------------------------------------------------------------------------------------------
// Round 6: the same attention on operands the QKV GEMM has ALREADY split (launch_gemm_p_qkv): nothing is converted here but
// the probabilities, and the K / V tiles come into LDS by LDS-DMA -- asynchronously, a whole phase ahead -- instead of through
// global loads -> 300 VALU conversions per thread and tile -> ds_write (round-5 counters: VALU issue 9.7 k of a wave's 37 k
// cycles, the matrix pipe 6.1 k, 45 % of the wave cycles parked at waits behind the synchronous staging).
//   qkvp  fp16 [plane h | l][Q | K | V][head][M rows][64 dims]   (128-byte rows: one DMA instruction = 8 keys = 1 KB contiguous)
// V stays ROW-MAJOR in LDS ([key][64 dims], as K); the V^T fragments of O^T += V^T P^T come out of it through the LDS transpose
// read ds_read_b64_tr_b16: the 16 lanes of a group hand in four rows of 16 dims (lane i: row i >> 2, dims 4 (i & 3) .. + 3) and
// lane i receives dim i of the four rows (tools/ubench/trread.hip prints the mapping) -- the rows may be ANY four keys, so a lane
// half takes exactly the keys its S^T accumulators hold ({4 lk .. + 3} and {8 + 4 lk .. + 3} of a 16-key group) and P^T goes back
// in from the registers as before; no transposed image, no transposing store anywhere.
// Key tiles, planes and every sum are those of flash_attn_f16x2_kernel: the same bits.  Rows of a tile beyond the document are the
// next document's (or row M - 1 again): finite, weighted exactly 0.
// Schedule of a tile t (two barriers, as before): [K(t) landed, barrier X] issue V(t) DMA, key biases, S^T(t) [V(t) landed,
// barrier Y] issue K(t + 1) DMA, soft-max, O^T += V^T P^T.  Every DMA batch has a whole compute phase to land in.
// ---------------------------------------------------------------------------------------------------------------
// one LDS-DMA instruction: lane i moves 16 bytes from [sbase + voff(i)] to LDS [lds_dst + 16 i]  (M0 saved / restored: compiler-reserved)
__device__ __forceinline__ void glds16(uint64_t sbase, uint32_t voff, uint32_t lds_dst) {
    uint32_t keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\t"
                 "global_load_lds_dwordx4 %1, %2\n\t"
                 "s_mov_b32 m0, %0"
                 : "=&s"(keep)
                 : "v"(voff), "s"(sbase), "s"(lds_dst)
                 : "memory");
}
// four keys x 16 dims, transposed: see above
typedef __fp16 fp16x4_raw __attribute__((__vector_size__(4 * sizeof(__fp16))));
__device__ __forceinline__ f16x8_t lds_tr_pair(const unsigned char* a0, const unsigned char* a1) {
    typedef _Float16 h4 __attribute__((ext_vector_type(4)));
    const fp16x4_raw x = __builtin_amdgcn_ds_read_tr16_b64_v4f16((__attribute__((address_space(3))) fp16x4_raw*)a0);
    const fp16x4_raw y = __builtin_amdgcn_ds_read_tr16_b64_v4f16((__attribute__((address_space(3))) fp16x4_raw*)a1);
    const h4 xh = __builtin_bit_cast(h4, x), yh = __builtin_bit_cast(h4, y);
    return __builtin_shufflevector(xh, yh, 0, 1, 2, 3, 4, 5, 6, 7);
}

// KT = keys per tile: 128 (two workgroups per CU: 66 KB of LDS each) or 64 (ASPIRE_HIP_ATTN=p64: 33 KB and 32 accumulator registers fewer -- three per CU;
// other tile edges, so other online-soft-max groupings: equal to the 128-key form to rounding, not bit for bit)
template <int KT, bool BIAS>
__device__ __forceinline__ void flash_attn_p_body(const unsigned char* __restrict__ qkvp, const int64_t* __restrict__ mask,
                                                  float* __restrict__ ctx, int L, int H, void* __restrict__ ctxp, int64_t rows,
                                                  const float* __restrict__ rel_bias, int rel_span) {
    constexpr int NRB = KT / 32;                                               // 32-key blocks per tile
    __shared__ __attribute__((aligned(16))) unsigned char Kp[2][KT * 128];    // [plane][key][64 dims fp16], piece ^ ((key >> 1) & 7)
    __shared__ __attribute__((aligned(16))) unsigned char Vp[2][KT * 128];    // [plane][key][64 dims fp16], piece ^ 4 ((key >> 1) & 1)
    __shared__ float kbias[KT];
    __shared__ float rtab[BIAS ? kRelTab : 1];
    const int tid = threadIdx.x, lane = tid & 63, lr = lane & 31, lk = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int qblocks = (L + 127) / 128;
    uint32_t wl;
    {
        const uint32_t nb = gridDim.x, bid = blockIdx.x, x = bid & 7, q8 = nb >> 3, r8 = nb & 7;
        wl = x * q8 + (x < r8 ? x : r8) + (bid >> 3);
    }
    const int qb = wl % qblocks, h = (wl / qblocks) % H, b = wl / (qblocks * H);
    const int64_t doc0 = (int64_t)b * L;                               // first row of the document
    const int q_row = qb * 128 + wave * 32 + lr;                       // this lane's query
    const bool q_ok = q_row < L;
    const float* rq = nullptr;                                          // BIAS: this lane's bias of key j (log2 units) at rq[j]
    if constexpr (BIAS) {
        stage_rel_bias(rtab, rel_bias, rel_span, h, L, tid);            // (read behind tile 0's barriers X and Y)
        rq = rtab + (L - 1 - min(q_row, L - 1));
    }
    const size_t plane_b = (size_t)3 * H * rows * 128;                 // bytes of one plane
    f16x8_t qh[4], ql[4];                                              // k step ks: dims 16 ks + 8 lk .. + 7 = piece 2 ks + lk of the row
    {
        const unsigned char* qp = qkvp + ((size_t)h * rows + (size_t)(doc0 + min(q_row, L - 1))) * 128 + 16 * lk;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            qh[ks] = *reinterpret_cast<const f16x8_t*>(qp + 32 * ks);
            ql[ks] = *reinterpret_cast<const f16x8_t*>(qp + plane_b + 32 * ks);
        }
    }
    f32x16 o[2];
#pragma unroll
    for (int mb = 0; mb < 2; ++mb)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[mb][r] = 0.f;
    float m_run = -INFINITY, l_run = 0.f;
    constexpr float kScaleLog2 = 0.125f * 1.44269504088896340736f;
    const uint32_t k_rd = lr * 128 + 16 * (lk ^ ((lr >> 1) & 7));
    // V transpose read: lane = (lk, dim half dh, i): hands in row 4 lk + (i >> 2) (+ 8 for the second read) of a 16-key group, dims 32 mb + 16 dh + 4 (i & 3) ..:
    // piece 4 mb + 2 dh + ((i & 3) >> 1), byte 8 (i & 1) in it; the piece is XORed with 4 ((key >> 1) & 1) = 4 ((i >> 3) & 1): keys two apart, 256 B
    // apart in the image, sit in different halves of the bank row
    const int vi = lane & 15, vdh = (lane >> 4) & 1;
    const uint32_t v_rd = (4 * lk + (vi >> 2)) * 128 + 16 * ((2 * vdh + ((vi & 3) >> 1)) ^ (4 * ((vi >> 3) & 1))) + 8 * (vi & 1);
    const uint32_t lds_k = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) unsigned char*)&Kp[0][0];
    const uint32_t lds_v = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) unsigned char*)&Vp[0][0];
    const int n_tiles = (L + KT - 1) / KT;
    // wave w moves keys 32 w .. 32 w + 31 of both planes of K (and of V), 8 keys per instruction: lane i -> key 8 c + (i >> 3), LDS piece i & 7 =
    // the row's piece (i & 7) ^ swizzle(key)
    const uint64_t k_base = (uint64_t)(uintptr_t)qkvp + ((size_t)(H + h) * rows) * 128;
    const uint64_t v_base = (uint64_t)(uintptr_t)qkvp + ((size_t)(2 * H + h) * rows) * 128;
    auto issue_kv = [&](int t, bool is_v) {
        const int64_t g = doc0 + (int64_t)t * KT;
#pragma unroll
        for (int c = 0; c < KT / 32; ++c) {
            const int key = (KT / 4) * wave + 8 * c + (lane >> 3);
            const int64_t row = min(g + key, rows - 1);
            const int sw = is_v ? 4 * ((key >> 1) & 1) : (key >> 1) & 7;
            const uint32_t voff = (uint32_t)(row * 128) + 16 * ((lane & 7) ^ sw);      // (< 4 GB per head: launch_gemm_p_qkv checks)
#pragma unroll
            for (int pl = 0; pl < 2; ++pl)
                glds16((is_v ? v_base : k_base) + pl * plane_b, voff, (is_v ? lds_v : lds_k) + pl * (KT * 128) + ((KT / 4) * wave + 8 * c) * 128);
        }
    };

    issue_kv(0, false);
    for (int t = 0; t < n_tiles; ++t) {
        const int k0 = t * KT;
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");               // X: this wave's pieces of K(t) have landed ...
        __syncthreads();                                               // ... everybody's; and everybody is past PV(t - 1): the V image is free
        issue_kv(t, true);
        if (tid < KT) {
            const int kk = k0 + tid;
            kbias[tid] = key_bias_log2(mask + (size_t)doc0, kk, L);      // (tile padding: the next document's rows)
        }
        // ---- S^T tile: 4 blocks of 32 keys x this wave's 32 queries; per k step the products l.h, h.l, h.h ----
        f32x16 sacc[NRB];
        const f32x16 zero16 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        // (consecutive MFMAs go to DIFFERENT accumulators -- the three products of a term run across the four key blocks -- so that none waits
        // for its predecessor's result; every accumulator still takes its products in the order l.h, h.l, h.h: the same sums)
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            f16x8_t kh[NRB], kl[NRB];
#pragma unroll
            for (int rb = 0; rb < NRB; ++rb) {
                const uint32_t at = (k_rd + rb * 32 * 128) ^ (32 * ks);
                kh[rb] = *reinterpret_cast<const f16x8_t*>(&Kp[0][at]);
                kl[rb] = *reinterpret_cast<const f16x8_t*>(&Kp[1][at]);
            }
#pragma unroll
            for (int rb = 0; rb < NRB; ++rb) sacc[rb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(kl[rb], qh[ks], ks == 0 ? zero16 : sacc[rb], 0, 0, 0);
#pragma unroll
            for (int rb = 0; rb < NRB; ++rb) sacc[rb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(kh[rb], ql[ks], sacc[rb], 0, 0, 0);
#pragma unroll
            for (int rb = 0; rb < NRB; ++rb) sacc[rb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(kh[rb], qh[ks], sacc[rb], 0, 0, 0);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");               // Y: this wave's pieces of V(t) have landed ...
        __syncthreads();                                               // ... everybody's, the key biases too; and everybody is past S^T(t): the K image is free
        if (t + 1 < n_tiles) issue_kv(t + 1, false);
        // ---- online soft-max over this tile's keys (registers of this lane + the other half-wave) -------------
        float tmax = -INFINITY;
#pragma unroll
        for (int rb = 0; rb < NRB; ++rb)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int key = 32 * rb + 8 * (r >> 2) + 4 * lk + (r & 3);
                if constexpr (BIAS)
                    sacc[rb][r] = fmaf(sacc[rb][r], kScaleLog2, rq[k0 + key]) + kbias[key];
                else
                    sacc[rb][r] = fmaf(sacc[rb][r], kScaleLog2, kbias[key]);
                tmax = fmaxf(tmax, sacc[rb][r]);
            }
        tmax = fmaxf(tmax, lane_xor<32>(tmax));
        const float m_new = fmaxf(m_run, tmax);
        const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);     // exp2(-inf) = 0 on the first tile
        float psum = 0.f;
#pragma unroll
        for (int rb = 0; rb < NRB; ++rb)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                sacc[rb][r] = __builtin_amdgcn_exp2f(sacc[rb][r] - m_new);
                psum += sacc[rb][r];
            }
        l_run = fmaf(l_run, alpha, psum);
        m_run = m_new;
#pragma unroll
        for (int mb = 0; mb < 2; ++mb)
#pragma unroll
            for (int r = 0; r < 16; ++r) o[mb][r] *= alpha;
        // ---- O^T += V^T P^T: registers 8 g .. 8 g + 7 of S^T block rb are the 8 keys of k step 2 rb + g in this lane half: keys
        // 16 s16 + {4 lk .. + 3} and 16 s16 + 8 + {4 lk .. + 3} -- the two transpose reads of the V^T fragment take exactly those rows ----
#pragma unroll
        for (int rb = 0; rb < NRB; ++rb)
#pragma unroll
            for (int g2 = 0; g2 < 2; ++g2) {
                const float pv[8] = {sacc[rb][8 * g2 + 0], sacc[rb][8 * g2 + 1], sacc[rb][8 * g2 + 2], sacc[rb][8 * g2 + 3],
                                     sacc[rb][8 * g2 + 4], sacc[rb][8 * g2 + 5], sacc[rb][8 * g2 + 6], sacc[rb][8 * g2 + 7]};
                f16x8_t ph, pl;
                split8_f16(pv, ph, pl);
                const int s16 = 2 * rb + g2;
                f16x8_t vh[2], vl[2];
#pragma unroll
                for (int mb = 0; mb < 2; ++mb) {
                    // rows 16 s16 + 4 lk + (i >> 2) and + 8: (key >> 1) & 1 is the same for both ((i >> 3) & 1: 16 s16, 4 lk and 8 leave bit 1 alone);
                    // dims 32 mb ..: pieces 4 mb .. -> ^ (64 mb) on the byte offset
                    const uint32_t at = (v_rd + s16 * 16 * 128) ^ (64 * mb);
                    vh[mb] = lds_tr_pair(&Vp[0][at], &Vp[0][at + 8 * 128]);
                    vl[mb] = lds_tr_pair(&Vp[1][at], &Vp[1][at + 8 * 128]);
                }
                // (the two dim blocks alternate: no MFMA directly behind the one whose result it accumulates onto)
#pragma unroll
                for (int mb = 0; mb < 2; ++mb) o[mb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vl[mb], ph, o[mb], 0, 0, 0);
#pragma unroll
                for (int mb = 0; mb < 2; ++mb) o[mb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vh[mb], pl, o[mb], 0, 0, 0);
#pragma unroll
                for (int mb = 0; mb < 2; ++mb) o[mb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vh[mb], ph, o[mb], 0, 0, 0);
            }
    }
    // ---- normalise and store (as flash_attn_f16x2_kernel) --------------------------------------------------------
    const float l_tot = l_run + lane_xor<32>(l_run);
    const float inv = 1.0f / l_tot;
    if (ctxp) {
#pragma unroll
        for (int mb = 0; mb < 2; ++mb)
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                float x[8];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float fa = o[mb][8 * t + e] * inv, fb = o[mb][8 * t + 4 + e] * inv;
                    auto r = __builtin_amdgcn_permlane32_swap(__builtin_bit_cast(int, fa), __builtin_bit_cast(int, fb), false, false);
                    const int x0 = r[0], x1 = r[1];
                    x[e] = __builtin_bit_cast(float, x0);
                    x[4 + e] = __builtin_bit_cast(float, x1);
                }
                if (q_ok) p_store8_at(ctxp, p_slot8((uint32_t)rows, (uint32_t)(doc0 + q_row), (uint32_t)(h * 64 + 32 * mb + 16 * t + 8 * lk)), x);
            }
    } else if (q_ok) {
        float* op = ctx + ((size_t)doc0 + q_row) * kD + h * 64;
#pragma unroll
        for (int mb = 0; mb < 2; ++mb)
#pragma unroll
            for (int g4 = 0; g4 < 4; ++g4)
                *reinterpret_cast<float4*>(op + 32 * mb + 8 * g4 + 4 * lk) =
                    make_float4(o[mb][4 * g4 + 0] * inv, o[mb][4 * g4 + 1] * inv, o[mb][4 * g4 + 2] * inv, o[mb][4 * g4 + 3] * inv);
    }
}

template <bool BIAS>
__global__ void __launch_bounds__(256, 2) flash_attn_p_kernel(const unsigned char* __restrict__ qkvp, const int64_t* __restrict__ mask,
                                                              float* __restrict__ ctx, int L, int H, void* __restrict__ ctxp, int64_t rows,
                                                              const float* __restrict__ rel_bias, int rel_span) {
    flash_attn_p_body<128, BIAS>(qkvp, mask, ctx, L, H, ctxp, rows, rel_bias, rel_span);
}
#ifndef ASPIRE_ATTN64_WAVES      // (experiment builds: 2 = leave a third of the SIMD's registers to another stream's GEMM waves)
#define ASPIRE_ATTN64_WAVES 3
#endif
__global__ void __launch_bounds__(256, ASPIRE_ATTN64_WAVES) flash_attn_p64_kernel(const unsigned char* __restrict__ qkvp, const int64_t* __restrict__ mask,
                                                                float* __restrict__ ctx, int L, int H, void* __restrict__ ctxp, int64_t rows) {
    flash_attn_p_body<64, false>(qkvp, mask, ctx, L, H, ctxp, rows, nullptr, 0);
}

// Attention of the CLS query alone, one workgroup per (document, head): softmax_j(q . k_j / 8 + (mask_j ? 0 : finfo.min)) v_j over the
// document's L <= 512 keys, in fp32 (the scores and the mask bias as softmax_mask_kernel forms them).  Q / K / V come from the fp32 qkv
// [rows, 2304] of the round-2 / f32 / f16x2 forms, or (qkvp != NULL) from the planes [plane h | l][Q | K | V][head][rows][64] fp16 that
// launch_gemm_p_qkv writes for flash_attn_p_kernel.  ctx [B, 768]: head h at columns 64 h .. + 63.
__device__ __forceinline__ void cls_attn_row(const float* qkv, const unsigned char* qkvp, int which, int H, int h, int64_t rows, int64_t row,
                                             float (&v)[64]) {
    if (qkvp) {
        const size_t plane_b = (size_t)3 * H * rows * 128;
        const unsigned char* p = qkvp + ((size_t)(which * H + h) * rows + row) * 128;
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            const f16x8_t hi = *reinterpret_cast<const f16x8_t*>(p + 16 * c), lo = *reinterpret_cast<const f16x8_t*>(p + plane_b + 16 * c);
#pragma unroll
            for (int e = 0; e < 8; ++e) v[8 * c + e] = (float)hi[e] + (float)lo[e];
        }
    } else {
        const float* p = qkv + row * 3 * kD + which * kD + h * 64;
#pragma unroll
        for (int c = 0; c < 16; ++c) {
            const float4 t = *reinterpret_cast<const float4*>(p + 4 * c);
            v[4 * c] = t.x, v[4 * c + 1] = t.y, v[4 * c + 2] = t.z, v[4 * c + 3] = t.w;
        }
    }
}
__device__ __forceinline__ float cls_attn_elem(const float* qkv, const unsigned char* qkvp, int which, int H, int h, int64_t rows, int64_t row, int d) {
    if (qkvp) {
        const unsigned char* p = qkvp + ((size_t)(which * H + h) * rows + row) * 128 + 2 * d;
        return (float)*reinterpret_cast<const _Float16*>(p) + (float)*reinterpret_cast<const _Float16*>(p + (size_t)3 * H * rows * 128);
    }
    return qkv[row * 3 * kD + which * kD + h * 64 + d];
}
__global__ void __launch_bounds__(256) cls_attn_kernel(const float* __restrict__ qkv, const unsigned char* __restrict__ qkvp,
                                                       const int64_t* __restrict__ mask, float* __restrict__ ctx, int L, int H, int64_t rows) {
    __shared__ float qs[64];
    __shared__ float pr[512];
    __shared__ float red[4];
    __shared__ float part[4][64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int h = (int)(blockIdx.x % H);
    const int64_t b = blockIdx.x / H, doc0 = b * L;
    if (tid < 64) qs[tid] = cls_attn_elem(qkv, qkvp, 0, H, h, rows, doc0, tid);
    __syncthreads();
    // scores: thread t takes keys t and t + 256
    float m = -INFINITY;
    for (int j = tid; j < L; j += 256) {
        float k[64];
        cls_attn_row(qkv, qkvp, 1, H, h, rows, doc0 + j, k);
        float s = 0.f;
#pragma unroll
        for (int d = 0; d < 64; ++d) s = fmaf(qs[d], k[d], s);
        s = s * 0.125f + (mask[doc0 + j] != 0 ? 0.f : -3.4028234663852886e38f);
        pr[j] = s;
        m = fmaxf(m, s);
    }
    m = wave_max(m);
    if (lane == 0) red[wave] = m;
    __syncthreads();
    m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    __syncthreads();
    float sum = 0.f;
    for (int j = tid; j < L; j += 256) {
        const float e = expf(pr[j] - m);
        pr[j] = e;
        sum += e;
    }
    sum = wave_sum(sum);
    if (lane == 0) red[wave] = sum;
    __syncthreads();
    const float inv = 1.0f / ((red[0] + red[1]) + (red[2] + red[3]));
    // context: wave w sums keys w, w + 4, ..; lane = dim
    float acc = 0.f;
    for (int j = wave; j < L; j += 4) acc = fmaf(pr[j], cls_attn_elem(qkv, qkvp, 2, H, h, rows, doc0 + j, lane), acc);
    part[wave][lane] = acc;
    __syncthreads();
    if (tid < 64) ctx[b * kD + h * 64 + tid] = ((part[0][tid] + part[1][tid]) + (part[2][tid] + part[3][tid])) * inv;
}

}  // namespace

// rel_bias (all launchers below but the CLS query's): NULL = BertModel's attention, the kernels instantiated without the bias
int launch_softmax_mask(float* s, const int64_t* mask, int64_t rows, int L, int ld, int rows_per_doc, float scale, const float* rel_bias,
                        int rel_span, hipStream_t st) {
    const dim3 grid((unsigned)((rows + 3) / 4));
    if (rel_bias)
        hipLaunchKernelGGL(softmax_mask_kernel<true>, grid, dim3(256), 0, st, s, mask, rows, L, ld, rows_per_doc, scale, rel_bias, rel_span);
    else
        hipLaunchKernelGGL(softmax_mask_kernel<false>, grid, dim3(256), 0, st, s, mask, rows, L, ld, rows_per_doc, scale, rel_bias, rel_span);
    ASPIRE_LAUNCH_OK();
    return ASPIRE_OK;
}

// the fused kernels: one workgroup per (document, head, 128 queries)
int launch_flash_attn(const float* qkv, const int64_t* mask, float* ctx, int64_t B, int L, int H, void* ctxp, int64_t rows, bool f32,
                      const float* rel_bias, int rel_span, hipStream_t st) {
    const dim3 grid((unsigned)(B * H) * (unsigned)((L + 127) / 128));
    if (f32 && rel_bias)
        hipLaunchKernelGGL(flash_attn_f32_kernel<true>, grid, dim3(256), 0, st, qkv, mask, ctx, L, H, ctxp, rows, rel_bias, rel_span);
    else if (f32)
        hipLaunchKernelGGL(flash_attn_f32_kernel<false>, grid, dim3(256), 0, st, qkv, mask, ctx, L, H, ctxp, rows, rel_bias, rel_span);
    else if (rel_bias)
        hipLaunchKernelGGL(flash_attn_f16x2_kernel<true>, grid, dim3(256), 0, st, qkv, mask, ctx, L, H, ctxp, rows, rel_bias, rel_span);
    else
        hipLaunchKernelGGL(flash_attn_f16x2_kernel<false>, grid, dim3(256), 0, st, qkv, mask, ctx, L, H, ctxp, rows, rel_bias, rel_span);
    ASPIRE_LAUNCH_OK();
    return ASPIRE_OK;
}

int launch_flash_attn_p(const unsigned char* qkvp, const int64_t* mask, float* ctx, int64_t B, int L, int H, void* ctxp, int64_t rows,
                        bool keys64, const float* rel_bias, int rel_span, hipStream_t st) {
    ASPIRE_REQUIRE(!(keys64 && rel_bias), ASPIRE_ERR_UNSUPPORTED,
                   "the 64-key attention form (ASPIRE_HIP_ATTN=p64) is not built with a relative-position bias");
    const dim3 grid((unsigned)(B * H) * (unsigned)((L + 127) / 128));
    if (keys64)
        hipLaunchKernelGGL(flash_attn_p64_kernel, grid, dim3(256), 0, st, qkvp, mask, ctx, L, H, ctxp, rows);
    else if (rel_bias)
        hipLaunchKernelGGL(flash_attn_p_kernel<true>, grid, dim3(256), 0, st, qkvp, mask, ctx, L, H, ctxp, rows, rel_bias, rel_span);
    else
        hipLaunchKernelGGL(flash_attn_p_kernel<false>, grid, dim3(256), 0, st, qkvp, mask, ctx, L, H, ctxp, rows, rel_bias, rel_span);
    ASPIRE_LAUNCH_OK();
    return ASPIRE_OK;
}

int launch_cls_attn(const float* qkv, const unsigned char* qkvp, const int64_t* mask, float* ctx, int64_t B, int L, int H, int64_t rows,
                    hipStream_t st) {
    hipLaunchKernelGGL(cls_attn_kernel, dim3((unsigned)(B * H)), dim3(256), 0, st, qkv, qkvp, mask, ctx, L, H, rows);
    ASPIRE_LAUNCH_OK();
    return ASPIRE_OK;
}

}  // namespace aspire
