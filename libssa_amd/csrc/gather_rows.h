// gather_rows.h -- what the device-side packers share (pairs_gather.hip,
// hits_gather.hip): a lane's sequence, anywhere in a byte pool, into its dword
// column of pairs.h's lane-interleaved layout.  Device code only.
//
// A sequence starts at any byte, so a lane reads ALIGNED dwords from the
// dword its sequence starts in and shifts neighbouring dwords together
// (v_alignbyte): five dwords in, one dwordx4 and one dword load, four output
// dwords = 16 codes out.  No load is unaligned and none depends on another.
//
// Padding is decided by INDEX: a byte at or past the lane's length becomes
// kPairsPad whatever the pool holds there (the next sequence, usually).  A
// lane loads only blocks that hold one of its own bytes, so nothing is read
// further than kGatherPoolPad behind a pool.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "pairs.h"

namespace ssa {
namespace {

constexpr uint32_t kWaves = 4;                       // waves per group: they take the 16-code blocks in turn
constexpr uint32_t kPad4 = kPairsPad * 0x01010101u;

struct __attribute__((packed, aligned(4))) Dwords4 {
    uint32_t w[4];
};

// The lane's `len` codes at pool + start into its dword column dst[row * 64],
// rows [0, nrows) of the group, padded by index.
__device__ __forceinline__ void gather_rows(const uint8_t* pool, const uint64_t start, const uint32_t len,
                                            uint32_t* dst, const uint32_t nrows, const uint32_t wave) {
    const uint32_t sh = (uint32_t)start & 3;
    const uint32_t* src = (const uint32_t*)(pool + (start - sh));
    const uint32_t nblk = (nrows + 3) / 4;
    for (uint32_t b = wave; b < nblk; b += kWaves) {
        const uint64_t first = (uint64_t)b * 16;     // the block's first code
        uint32_t out[4] = {kPad4, kPad4, kPad4, kPad4};
        if (first < len) {
            const Dwords4 x = *(const Dwords4*)(src + (size_t)b * 4);
            const uint32_t y = src[(size_t)b * 4 + 4];
            out[0] = __builtin_amdgcn_alignbyte(x.w[1], x.w[0], sh);
            out[1] = __builtin_amdgcn_alignbyte(x.w[2], x.w[1], sh);
            out[2] = __builtin_amdgcn_alignbyte(x.w[3], x.w[2], sh);
            out[3] = __builtin_amdgcn_alignbyte(y, x.w[3], sh);
            const uint32_t left = min(len - (uint32_t)first, 16u);   // own codes in the block, 1..16
#pragma unroll
            for (uint32_t k = 0; k < 4; k++) {
                const uint32_t keep = left > 4 * k ? min(left - 4 * k, 4u) : 0u;   // own codes in dword k
                const uint32_t mask = keep >= 4 ? 0xffffffffu : (1u << (8 * keep)) - 1u;
                out[k] = (out[k] & mask) | (kPad4 & ~mask);
            }
        }
#pragma unroll
        for (uint32_t k = 0; k < 4; k++)
            if (b * 4 + k < nrows) dst[((size_t)b * 4 + k) * 64] = out[k];
    }
}

}  // namespace
}  // namespace ssa
