// pairs_banded.h -- the banded pair calls' device interface (pairs_banded.hip;
// host side: pairs_banded.cpp).  Packing, lanes, the mask bits,
// the four direction bits per cell and the walk's step (next_op) are
// pairs_ends.h's.  On top of them every lane has its band [lo, hi] of
// diagonals k = column - row, and every (group, strip) its range of swept
// column blocks:
//   band   [group][lane]                       int2 (lo, hi), clamped to [-qlen - 1, dlen + 1]
//   strips [group's s_row + strip]             BandStrip: the blocks the wave sweeps in that strip
//   dir    [group][strip][block - cb0][lane]   uint4 as pairs_ends.h's, swept blocks only
#pragma once
#include "pairs_ends.h"

namespace ssa {

// The int32 representative of minus infinity: H of a cell that does not exist.
// Every real value is inside +-2^29 (the device score bound), so it is below
// all of them, and a difference of any two values stays inside int32
// (pairs_banded.hip's header has the argument).
constexpr int32_t kBandNegInf = -(1 << 30);
// nruns of a lane whose walk stood on a cell outside what was stored
constexpr uint32_t kBandWalkLost = 0xffffffffu;

struct BandGroup {
    uint32_t t_row, q_row, b_row;   // as PairsGroup
    uint32_t ncb, nstrips;          // the group's extents (column blocks of the longest target, strips)
    uint32_t d_row;                 // first 64-lane uint4 row of the group in dir
    uint32_t s_row;                 // first entry of the group in strips
    uint32_t pad;
};

struct BandStrip {
    uint32_t cb0, ncb;              // the swept blocks [cb0, cb0 + ncb); ncb 0: nothing in the band
    uint32_t d_off;                 // the strip's first dir row, from the group's d_row
    uint32_t pad;
};

struct BandedArgs {
    const uint32_t* tres;
    const uint32_t* qres;
    int2* bnd;
    const BandGroup* groups;
    const BandStrip* strips;
    const uint2* lens;              // (qlen, dlen) per lane; (0, 0): unused
    const int2* band;               // (lo, hi) per lane
    const AlignLane* lanes;         // the walk: used, slot, cap
    const int8_t* mt;               // as PairsArgs::mt
    uint4* dir;                     // the align call: direction bits
    uint32_t* runs;                 // the walk: as AlignArgs::runs
    uint32_t* nruns;                // the walk: runs written per lane, or kBandWalkLost
    int2* out;                      // (score, end cell as col << 16 | row)
    int32_t gap_open, gap_extend;
    int32_t ends;                   // the mask, 0..15
    uint32_t ngroups;
};

// pass: 0 scores (banded_kernel<false>), 1 scores and directions (banded_kernel<true>), 2 the walk
hipError_t launch_pairs_banded(int pass, const BandedArgs& a, hipStream_t st);

}  // namespace ssa
