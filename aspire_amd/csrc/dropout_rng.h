// The training encoder's dropout: the generator, the keying and the keep rule, stated once for the device and the host (this header
// compiles as plain C++ too: a host program can print the words the kernels draw).  No rocRAND, no torch generator, no mask in memory:
// a mask is a pure function of (seed, step, site, element), formed again wherever it is needed.
//
// Generator   Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11): multipliers 0xD2511F53 / 0xCD9E8D57,
//             Weyl key increments 0x9E3779B9 / 0xBB67AE85, ten rounds of
//               c' = [hi(M1 c2) ^ c1 ^ k0, lo(M1 c2), hi(M0 c0) ^ c3 ^ k1, lo(M0 c0)]
//             with the key bumped between rounds.  Known answers (counter, key -> output):
//               0, 0                                                   -> 6627e8d5 e169c58d bc57ac4c 9b00dbd8
//               all ff, all ff                                         -> 408f276d 41c83b0e a20bc7c6 6d5451fd
//               243f6a88 85a308d3 13198a2e 03707344, a4093822 299f31d0 -> d16cfe09 94fdcceb 5001e420 24126ea1
// Keying      key = the 64-bit seed (low word, high word); counter = (block low, block high, site, step); block = e >> 2 and element
//             e takes output word e & 3.  e is the element's LOGICAL flat index in the tensor HuggingFace drops -- [B, L, 768] at the
//             hidden sites, [B, H, L, L] for the probabilities, not the tape's Lp-padded rows -- so a mask never depends on an
//             internal stride.  step is a uint32 the caller advances once per training forward.
// Sites       HuggingFace's call order: 0 after the embedding LayerNorm (p_hidden); per layer l: 1 + 3 l the soft-max probabilities
//             (p_attn), 2 + 3 l the out-projection's output before the residual (p_hidden), 3 + 3 l the FFN2 output before the
//             residual (p_hidden).
// Keep rule   keep iff word >= thr, thr = (uint32) floor((double) p 2^32); a kept element is multiplied by scale = 1.0f / (1.0f - p)
//             (fp32), a dropped one is 0.0f.  p in [0, 1); a site with p == 0 gets no launch at all.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define ASPIRE_HD __host__ __device__ __forceinline__
#else
#define ASPIRE_HD inline
#endif

namespace aspire {

struct Philox4 {
    uint32_t w[4];
};

ASPIRE_HD Philox4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
    constexpr uint32_t kM0 = 0xD2511F53u, kM1 = 0xCD9E8D57u, kW0 = 0x9E3779B9u, kW1 = 0xBB67AE85u;
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)kM0 * c0, p1 = (uint64_t)kM1 * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c0 = n0; c1 = (uint32_t)p1; c2 = n2; c3 = (uint32_t)p0;
        k0 += kW0; k1 += kW1;
    }
    return Philox4{{c0, c1, c2, c3}};
}

// One dropout site of one step: what a kernel needs to form the site's mask
struct DropSite {
    uint64_t seed;
    uint32_t step, site;
    uint32_t thr;       // keep iff word >= thr
    float scale;        // 1 / (1 - p)
};

// the four words of elements 4 block .. 4 block + 3
ASPIRE_HD Philox4 drop_block(const DropSite& d, uint64_t block) {
    return philox4x32_10((uint32_t)block, (uint32_t)(block >> 32), d.site, d.step, (uint32_t)d.seed, (uint32_t)(d.seed >> 32));
}

// word i < 4 of a block by selects (an indexed read of w would put the four words in scratch memory)
ASPIRE_HD uint32_t drop_word(const Philox4& r, uint32_t i) { return i == 0 ? r.w[0] : i == 1 ? r.w[1] : i == 2 ? r.w[2] : r.w[3]; }

ASPIRE_HD bool drop_keep(const DropSite& d, uint64_t e) { return drop_word(drop_block(d, e >> 2), (uint32_t)(e & 3)) >= d.thr; }

inline uint32_t drop_threshold(float p) { return (uint32_t)((double)p * 4294967296.0); }      // (p in [0, 1): floor, below 2^32)

inline DropSite drop_site(uint64_t seed, uint32_t step, uint32_t site, float p) {
    return DropSite{seed, step, site, drop_threshold(p), 1.0f / (1.0f - p)};
}

}  // namespace aspire
