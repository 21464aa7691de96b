// pairs_xdrop.h -- the X-drop pair calls' device interface (pairs_xdrop.hip;
// host side: pairs_xdrop.cpp).  Packing, groups, strips, bands
// and the end cell in out are pairs_banded.h's and pairs_local.h's: the end
// pass is the local score pass of a mode with a local end and a fixed or free
// begin (42, 43, 46, 47), and every cell's H, E and F are that pass's.  Only
// the end candidates differ: rows are visited in ascending order, a row whose
// greatest finite H lies more than xdrop below the best so far is the DROP ROW,
// and no row from it on holds a candidate.  On top of out the pass leaves
//   dropped [group][lane]   uint32: 1 where the lane met a drop row
//   entered [group]         uint32: strips the wave entered before it left the strip loop
#pragma once
#include "pairs_local.h"

namespace ssa {

// xdrop values from here on never stop a device pair: best - m stays below 2^30 (pairs_banded.h's bound)
constexpr int64_t kXdropMax = (int64_t)1 << 30;

struct XdropArgs {
    BandedArgs b;                   // b.ends: the canonical mode's four kFree* bits
    int32_t xdrop;                  // 0 .. kXdropMax
    uint32_t* dropped;
    uint32_t* entered;
};

// xdrop_kernel: local_kernel<false, false, true>'s sweep with the end candidates tracked row by row --
// (best, col << 16 | row) to out, 0xffffffff for no end cell (best is then 0)
hipError_t launch_pairs_xdrop(const XdropArgs& a, hipStream_t st);

}  // namespace ssa
