// hits_gather.h -- the device-side packer of ssa_amd_summarize_hits
// (hits_gather.hip; host side: hits_summary.cpp).  The d side
// of a hit already lies on the device, in the packed DB the search kernels
// read (DeviceDB::d_res); the q side is one of the query's few
// views.  The host uploads one descriptor per lane and the views once per
// call; hits_gather_kernel writes pairs.h's lane-interleaved qres / tres /
// lens from them, directly in front of the summary kernels on the same stream.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "pairs_banded.h"   // BandGroup: the pair groups of the chunk

namespace ssa {

// One lane's hit: the entry's global lane in the packed DB (group * 64 + lane
// of the group), its length, the query view and its length.  All zero: the
// lane is unused (all padding, lens (0, 0)).
struct HitDesc {
    uint32_t lane, dlen;
    uint32_t view, qlen;
};
static_assert(sizeof(HitDesc) == 16, "one descriptor per lane, 16 bytes");

constexpr uint32_t kHitsMaxViews = 8;     // views the per-call table has room for (a query has at most 6)
constexpr uint32_t kHitsCodes = 64;       // entries of the code table: compact code -> residue code or kPairsPad

// The per-call table in front of the view pool.
struct HitsTable {
    uint8_t code_of[kHitsCodes];          // DeviceDB::code_of, entry alpha and everything above kPairsPad
    uint32_t view_start[kHitsMaxViews];   // first byte of each view in the pool
};

struct HitsGatherArgs {
    const HitDesc* desc;          // [group][lane]
    const BandGroup* groups;      // t_row, q_row, ncb, nstrips of each pair group
    const HitsTable* table;
    const uint8_t* qpool;         // the views; 4-byte aligned, kGatherPoolPad readable bytes behind it
    const uint4* dres;            // DeviceDB::d_res, read only: [block][lane] 16 compact codes
    const uint2* dgroups;         // DeviceDB::d_groups, a GroupDesc (kernels.h) as (blk, ncols) per DB group
    uint32_t* qres;               // pairs.h's layout, written whole: the group's nstrips * 2 rows
    uint32_t* tres;               // and ncb rows
    uint2* lens;
    uint32_t ngroups;
};

hipError_t launch_hits_gather(const HitsGatherArgs& a, hipStream_t st);

}  // namespace ssa
