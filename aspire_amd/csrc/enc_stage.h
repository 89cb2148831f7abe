// Staging of an fp32 operand tile onto the bf16 matrix pipe, shared by enc_gemm_bf16.hip (one plane: every element rounded to bf16 once)
// and enc_gemm_bf16x3.hip (three planes: x = x1 + x2 + x3, split3_bf16): the coalesced global loads, the register turn of a k-major
// operand, and the swizzled LDS image that the MFMA fragment reads take.  Device code only.
//
// The MFMA fragment is eight consecutive k of one row, so the LDS image of a plane of a tile is [k group of 8][row][8 bf16], 16 bytes
// per row.  A k-contiguous operand stores its float4 (four k of one row) as one 8-byte half of such a row.  A K-MAJOR operand (a row
// of global memory is a k-slice) is turned IN REGISTERS: a thread loads a 4 k x 4 row block as four float4 along the rows (coalesced:
// eight lanes cover 128 contiguous bytes of a k-slice), and writes each of its four rows' four consecutive k as one 8-byte store into
// the same image -- the scatter route; the fragment reads are then plain 16-byte reads, the same for every form.  (The other
// route, storing k-major and reading through the LDS transpose read, needs no register turn but a second read path; NOTES.md.)
// Rows are swizzled, row ^ ((row >> 3) & 3), the same in stores and reads: within an aligned group of four rows a permutation, so a
// fragment read (16 lanes = 16 consecutive rows = 256 bytes) stays conflict free, and the four-row stride of the turned stores
// (rows 4 m + i for eight lanes m) lands on eight distinct 16-byte slots of a 128-byte window instead of two.
#pragma once
#include "enc_types.h"

namespace aspire {
namespace {

typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));

// two fp32 -> one dword of two bf16 (low half = the first), round to nearest even
__device__ __forceinline__ uint32_t pack_bf16(float x, float y) {
    typedef __bf16 bf2 __attribute__((ext_vector_type(2)));
    typedef float f2 __attribute__((ext_vector_type(2)));
    const f2 v = {x, y};
    return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, bf2));
}

// two fp32 -> PLANES dwords of two bf16 each: the one rounding, or the three planes of split3_bf16 (common.h)
template <int PLANES>
__device__ __forceinline__ void to_planes(float x, float y, uint32_t (&p)[PLANES]) {
    static_assert(PLANES == 1 || PLANES == 3, "one rounding or the three-plane split");
    if constexpr (PLANES == 1) p[0] = pack_bf16(x, y);
    else split3_bf16(x, y, p[0], p[1], p[2]);
}

// p[0 .. 4) where n (<= 0: none) elements from p on are valid; the rest zero.  p is 16-byte aligned.
__device__ __forceinline__ float4 load4_valid(const float* p, int n) {
    if (n >= 4) return *reinterpret_cast<const float4*>(p);
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (n > 0) v.x = p[0];
    if (n > 1) v.y = p[1];
    if (n > 2) v.z = p[2];
    return v;
}

__device__ __forceinline__ int swizzle_row(int r) { return r ^ ((r >> 3) & 3); }

// One operand's tile, ROWS x BK k, from global memory to registers and from registers to its LDS image of PLANES planes.  K_MAJOR: the
// operand is [K][ld] with the tile's rows along the contiguous dimension.  `rows` / `K`: the operand's valid extent; r0 / k0: the
// tile's origin.  `tid`: the thread's index among the 256 that stage the tile; a k-major tile has (ROWS / 4) (BK / 4) blocks and the
// threads beyond them stage nothing (the caller may hand them another operand's blocks).
template <int ROWS, bool K_MAJOR, int BK, int PLANES>
struct StageRegs {
    static constexpr int kGroups = BK / 8;                                         // k groups of eight
    static constexpr int kPlane = ROWS * 4 + 8;                                    // dwords of one k group: ROWS x 16 bytes + 32 bytes, so that the groups' stores fall in different quarters of a 128-byte window
    static constexpr int N4 = K_MAJOR ? 4 : ROWS * (BK / 4) / 256;                 // float4 per thread
    static constexpr int kUnits = (ROWS / 4) * (BK / 4);                           // K_MAJOR: 4 x 4 blocks of the tile
    static_assert(BK % 8 == 0 && N4 >= 1 && kUnits <= 256 && kUnits % 16 == 0, "tile / thread layout");
    float4 v[N4];

    __device__ __forceinline__ void load(const float* X, int ld, int rows, int K, int r0, int k0, int tid) {
        if constexpr (K_MAJOR) {
            const bool active = kUnits >= 256 || (unsigned)tid < (unsigned)kUnits;
            const int m4 = ((tid >> 4) % (ROWS / 32)) * 8 + (tid & 7), kq = ((tid >> 4) / (ROWS / 32)) * 2 + ((tid >> 3) & 1);
            const int r = r0 + 4 * m4;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int k = k0 + 4 * kq + j;
                v[j] = load4_valid(X + (size_t)k * ld + r, active && k < K ? rows - r : 0);
            }
        } else {
#pragma unroll
            for (int p = 0; p < N4; ++p) {
                const int idx = tid + 256 * p, row = idx / (BK / 4), k4 = idx % (BK / 4);
                const int r = r0 + row, k = k0 + 4 * k4;
                v[p] = load4_valid(X + (size_t)r * ld + k, r < rows ? K - k : 0);
            }
        }
    }
    // S: the buffer's image [PLANES][kGroups][kPlane]
    __device__ __forceinline__ void store(uint32_t (*S)[kGroups][kPlane], int tid) const {
        if constexpr (K_MAJOR) {
            if (kUnits < 256 && (unsigned)tid >= (unsigned)kUnits) return;
            const int m4 = ((tid >> 4) % (ROWS / 32)) * 8 + (tid & 7), kq = ((tid >> 4) / (ROWS / 32)) * 2 + ((tid >> 3) & 1);
            // the turn: k-slice j gives (rows 0, 1) and (rows 2, 3) at k = j as two dwords per plane, converted where they lie; row i
            // then takes its halves of the four slices' dwords (integer selects: no float leaves its float4)
            uint32_t p01[4][PLANES], p23[4][PLANES];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                to_planes<PLANES>(v[q].x, v[q].y, p01[q]);
                to_planes<PLANES>(v[q].z, v[q].w, p23[q]);
            }
            auto lo = [](uint32_t a, uint32_t b) { return (a & 0xffffu) | (b << 16); };
            auto hi = [](uint32_t a, uint32_t b) { return (a >> 16) | (b & 0xffff0000u); };
#pragma unroll
            for (int pl = 0; pl < PLANES; ++pl) {
                uint32_t* base = &S[pl][kq >> 1][2 * (kq & 1)];
                *reinterpret_cast<uint2*>(base + 4 * swizzle_row(4 * m4 + 0)) = make_uint2(lo(p01[0][pl], p01[1][pl]), lo(p01[2][pl], p01[3][pl]));
                *reinterpret_cast<uint2*>(base + 4 * swizzle_row(4 * m4 + 1)) = make_uint2(hi(p01[0][pl], p01[1][pl]), hi(p01[2][pl], p01[3][pl]));
                *reinterpret_cast<uint2*>(base + 4 * swizzle_row(4 * m4 + 2)) = make_uint2(lo(p23[0][pl], p23[1][pl]), lo(p23[2][pl], p23[3][pl]));
                *reinterpret_cast<uint2*>(base + 4 * swizzle_row(4 * m4 + 3)) = make_uint2(hi(p23[0][pl], p23[1][pl]), hi(p23[2][pl], p23[3][pl]));
            }
        } else {
#pragma unroll
            for (int p = 0; p < N4; ++p) {
                const int idx = tid + 256 * p, row = idx / (BK / 4), k4 = idx % (BK / 4);
                uint32_t xy[PLANES], zw[PLANES];
                to_planes<PLANES>(v[p].x, v[p].y, xy);
                to_planes<PLANES>(v[p].z, v[p].w, zw);
#pragma unroll
                for (int pl = 0; pl < PLANES; ++pl)
                    *reinterpret_cast<uint2*>(&S[pl][k4 >> 1][4 * swizzle_row(row) + 2 * (k4 & 1)]) = make_uint2(xy[pl], zw[pl]);
            }
        }
    }
};

}  // namespace
}  // namespace aspire
