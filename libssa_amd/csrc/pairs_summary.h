// pairs_summary.h -- the summary call's device interface (pairs_summary.hip;
// host side: pairs_summary.cpp).  Packing, groups, strips,
// bands and the end cell in out are pairs_banded.h's and pairs_local.h's.  On
// top of them the summary sweep carries two words beside every value
//   word A   identical << 16 | matched        M columns of the path so far, and those with equal codes
//   word B   q_begin << 16 | d_begin          where the path began
// and keeps, between strips, the bottom row's words of H and F:
//   rows   [group][col][lane]   uint4 (H's A, H's B, F's A, F's B), indexed as bnd
//   sum    [group][lane]        uint2 (A, B) of H at the lane's end cell; (0, 0): nothing captured
#pragma once
#include "pairs_local.h"

namespace ssa {

struct SummaryArgs {
    BandedArgs b;                   // b.out: the end-cell pass's (score, col << 16 | row), read only
    uint4* rows;                    // the row buffer of the words, beside b.bnd
    uint2* sum;                     // the lane's summary words
};

// summary_kernel<LB>: the score pass's sweep with the words, capturing by index at out's end cell; lb: the
// canonical mode has a local begin.  local: the mode has a local bit -- lanes with a score <= 0 capture nothing.
hipError_t launch_pairs_summary(bool lb, bool local, const SummaryArgs& a, hipStream_t st);

}  // namespace ssa
