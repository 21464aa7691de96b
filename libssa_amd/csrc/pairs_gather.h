// pairs_gather.h -- the device-side packer of the indexed pair call
// (ssa_amd_score_pairs_indexed; pairs_gather.hip).  The host
// uploads the two sequence pools once per call and one descriptor per lane;
// pairs_gather_kernel writes pairs.h's lane-interleaved qres / tres / lens
// from them, directly in front of pairs_kernel on the same stream.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "pairs.h"

namespace ssa {

// One lane's pair: byte offsets of its two sequences in their pools and the
// lengths.  (0, 0) lengths: the lane is unused (all padding, lens (0, 0)).
struct PairsDesc {
    uint64_t q_start, d_start;
    uint32_t qlen, dlen;
};
static_assert(sizeof(PairsDesc) == 24, "one descriptor per lane, 24 bytes");

// Bytes a pool's device copy is allocated past its end: the gather reads whole
// aligned dwords, five per block of 16 codes, so a lane's last block ends at
// most 19 bytes behind its sequence (pairs_gather.hip, gather_rows).
constexpr size_t kGatherPoolPad = 64;

struct GatherArgs {
    const PairsDesc* desc;        // [group][lane]
    const PairsGroup* groups;     // t_row, q_row, ncb, nstrips of each group
    const uint8_t* qpool;         // 4-byte aligned, kGatherPoolPad readable bytes behind each pool
    const uint8_t* dpool;
    uint32_t* qres;               // pairs.h's layout, written whole: the group's nstrips * 2 rows
    uint32_t* tres;               // and ncb rows
    uint2* lens;
    uint32_t ngroups;
};

hipError_t launch_pairs_gather(const GatherArgs& a, hipStream_t st);

}  // namespace ssa
