// pairs_ends.h -- the ends-free (semi-global) pair calls' device interface
// (pairs_ends.hip; host side: pairs_ends.cpp).  Packing,
// groups and lanes are pairs_align.h's.  The direction bits are its own: four
// per cell, because the walk keeps the state an affine gap needs
//   dir   [group][strip][col / 4][lane]   uint4: 4 columns (x, y, z, w) x 8 rows x 4 bits;
//                                         row r's nibble at bits 4 * (7 - r): kDir* below
#pragma once
#include "pairs_align.h"

namespace ssa {

// the mask bits of include/libssa_amd.h
constexpr int kFreeQBegin = 1, kFreeQEnd = 2, kFreeDBegin = 4, kFreeDEnd = 8;

// a cell's direction bits, directions()'s four (align.cpp)
constexpr uint32_t kDirLeft = 8;      // H took E (after the diagonal and F)
constexpr uint32_t kDirUp = 4;        // H took F (after the diagonal)
constexpr uint32_t kDirExtLeft = 2;   // E of the next column extends this cell's E (else it opens from its H)
constexpr uint32_t kDirExtUp = 1;     // F of the next row extends this cell's F

// The walk's step at a cell with bits d, entered by `last` (kOpM: through H --
// a diagonal step or the end cell): a gap goes on while its extension bit is
// set; else the cell's H decides, left first, then up, else diagonal.
__host__ __device__ inline uint32_t next_op(const uint32_t last, const uint32_t d) {
    if (last == kOpI && (d & kDirExtLeft)) return kOpI;
    if (last == kOpD && (d & kDirExtUp)) return kOpD;
    return (d & kDirLeft) ? kOpI : (d & kDirUp) ? kOpD : kOpM;
}

struct EndsArgs {
    const uint32_t* tres;
    const uint32_t* qres;
    int2* bnd;
    const AlignGroup* groups;       // the align call: d_row set (rows of 64 uint4); the score call: d_row unused
    const uint2* lens;              // (qlen, dlen) per lane; (0, 0): unused
    const AlignLane* lanes;         // the walk: used, slot, cap (the end cell comes from out)
    const int8_t* mt;               // as PairsArgs::mt
    uint4* dir;                     // the align call: direction bits
    uint32_t* runs;                 // the walk: as AlignArgs::runs
    uint32_t* nruns;                // the walk: runs written per lane
    int2* out;                      // (score, end cell as col << 16 | row -- meaningful for lengths < 65 536)
    int32_t gap_open, gap_extend;
    int32_t ends;                   // the mask, 0..15
    uint32_t ngroups;
};

// pass: 0 scores (ends_kernel<false>), 1 scores and directions (ends_kernel<true>), 2 the walk
hipError_t launch_pairs_ends(int pass, const EndsArgs& a, hipStream_t st);

}  // namespace ssa
