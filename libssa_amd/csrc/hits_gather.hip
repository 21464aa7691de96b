// hits_gather.hip -- hits_gather_kernel: packs one group of 64 search hits per
// workgroup into pairs.h's lane-interleaved layout, the d sides taken from the
// packed DB on the device (arguments: hits_gather.h; host side:
// hits_summary.cpp).
//
// Lane l of every wave owns pair l of the group; the four waves take the
// 16-code blocks in turn, as pairs_gather_kernel does, and each store writes
// one whole 64-lane row of the output.
//
// The q side is a query view in the view pool: gather_rows, as it is.
//
// The d side needs neither alignbyte nor a second load: the packed DB keeps
// columns 16 b .. 16 b + 15 of a lane in 16 consecutive, 16-byte aligned bytes
// (engine.cpp build_host_pack), so block b of the lane's entry is the one
// uint4 dres[(dgroups[g].blk + b) * 64 + (lane & 63)], g = lane / 64.  Its 16
// COMPACT codes become residue codes through the table (held in LDS, byte
// reads).  The class-coded copy of the DB (d_res_cls) depends on the last
// query and is never read here.
//
// Padding is decided by INDEX.  A lane loads block b only if 16 b < dlen: the
// pair group's ncb follows the longest d of the PAIR group, the DB group's
// block count the longest entry of the DB group, and a short entry's DB group
// ends long before a long neighbour's columns do -- so no block is read that
// holds none of the lane's own codes, and nothing behind the last DB group.
// Bytes at or past dlen become kPairsPad under a mask from the length,
// whatever the DB's own padding column translates to.  All nstrips * 2 and ncb
// rows of the group and the lens of all 64 lanes are written: no memset pass.
#include "gather_rows.h"
#include "hits_gather.h"
#include "launch.h"

namespace ssa {
namespace {

// four compact codes of a dword -> their residue codes
__device__ __forceinline__ uint32_t translate4(const uint8_t* code, const uint32_t w) {
    return (uint32_t)code[w & (kHitsCodes - 1)] | (uint32_t)code[(w >> 8) & (kHitsCodes - 1)] << 8 |
           (uint32_t)code[(w >> 16) & (kHitsCodes - 1)] << 16 | (uint32_t)code[(w >> 24) & (kHitsCodes - 1)] << 24;
}

__global__ void __launch_bounds__(64 * kWaves) hits_gather_kernel(const HitsGatherArgs a) {
    __shared__ uint8_t s_code[kHitsCodes];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t g = blockIdx.x;
    if (threadIdx.x < kHitsCodes) s_code[threadIdx.x] = a.table->code_of[threadIdx.x];
    __syncthreads();
    const BandGroup G = a.groups[g];
    const HitDesc D = a.desc[(size_t)g * 64 + lane];
    if (wave == 0) a.lens[(size_t)g * 64 + lane] = make_uint2(D.qlen, D.dlen);
    gather_rows(a.qpool, a.table->view_start[D.view & (kHitsMaxViews - 1)], D.qlen,
                a.qres + ((size_t)G.q_row * 64 + lane), G.nstrips * 2, wave);

    // ---- the d side: aligned 16-code blocks of the packed DB
    const uint4* src = a.dres + ((size_t)a.dgroups[D.lane >> 6].x * 64 + (D.lane & 63));
    uint32_t* dst = a.tres + ((size_t)G.t_row * 64 + lane);
    const uint32_t nrows = G.ncb, nblk = (nrows + 3) / 4;
    for (uint32_t b = wave; b < nblk; b += kWaves) {
        const uint32_t first = b * 16;               // the block's first code
        uint32_t out[4] = {kPad4, kPad4, kPad4, kPad4};
        if (first < D.dlen) {
            const uint4 x = src[(size_t)b * 64];
            out[0] = translate4(s_code, x.x);
            out[1] = translate4(s_code, x.y);
            out[2] = translate4(s_code, x.z);
            out[3] = translate4(s_code, x.w);
            const uint32_t left = min(D.dlen - first, 16u);          // own codes in the block, 1..16
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

hipError_t launch_hits_gather(const HitsGatherArgs& a, hipStream_t st) {
    if (a.ngroups == 0) return hipSuccess;
    (void)ssa_launch((const void*)&hits_gather_kernel, dim3(a.ngroups), dim3(64 * kWaves), 0, st, a);
    return hipGetLastError();
}

}  // namespace ssa
