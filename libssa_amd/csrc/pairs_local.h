// pairs_local.h -- the local pair calls' device interface (pairs_local.hip;
// host side: pairs_local.cpp).  Packing, groups, strips, bands
// and the four direction bits per cell are pairs_banded.h's.  On top of them
// the mode has two bits, and a local begin keeps one more bit per cell:
//   stop   [group][strip][block - cb0][lane]   uint32 beside dir's uint4 (the same row index): the cell
//                                              (row r of the strip, column k of the block) at bit 31 - 8 k - r
#pragma once
#include "pairs_banded.h"

namespace ssa {

// the mode bits of include/libssa_amd.h beside the four kFree* ones
constexpr int kLocalBegin = 16, kLocalEnd = 32;

// A local begin's fifth bit in the host path's direction byte: max(D, E, F) <= 0, the walk stops here.
constexpr uint32_t kDirStop = 16;

struct LocalArgs {
    BandedArgs b;                   // b.ends: the canonical mode's four kFree* bits
    uint32_t* stop;                 // the align call under a local begin: STOP bits
};

// pass 0: the score pass, local_kernel<false, LB, LE> -- (score, end cell) to out; under a local end the end
//         cell is the smallest (column, row) among all existing real cells with the greatest H
// pass 1: the direction pass, local_kernel<true, LB, LE> -- dir and, under a local begin, stop; writes out
//         only without a local end (then it tracks the end cell as banded_kernel<true> does)
// pass 2: local_walk_kernel, from out's end cells; lanes with a score <= 0 walk nowhere
hipError_t launch_pairs_local(int pass, int mode, const LocalArgs& a, hipStream_t st);

}  // namespace ssa
