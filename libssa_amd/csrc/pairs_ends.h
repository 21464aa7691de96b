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

// ------------------------------------------- shared with pairs_banded.cpp
// (host side, defined in pairs_ends.cpp)
struct EndCell {
    int64_t score;
    size_t q_end, d_end;
};
// the tie rule between the kept last-row and last-column candidates
EndCell ends_pick_cell(int64_t row_best, size_t row_col, int64_t col_best, size_t col_row, size_t qn, size_t dn);
// the closed form of a pair with an empty side
int64_t ends_empty_score(int ends, size_t qn, size_t dn, int64_t Q, int64_t R);
// region and text from the end cell and the walk's runs (leading run where a begin is not free)
uint32_t ends_finish_alignment(int ends, size_t q_end, size_t d_end, std::vector<uint32_t>& runs, uint64_t region[4],
                               char* text);
// ssa_amd_score_pairs' argument checks, and the mask's
bool ends_args_ok(int ends, const uint8_t* qc, const uint64_t* qoff, const uint8_t* dc, const uint64_t* doff,
                  size_t n);
// what the int32 kernels take: device or not, the residue limit behind the 2^29 bound, the compact matrix
struct EndsRouting {
    bool device = false;
    int dev_id = -1;
    hipStream_t stream = nullptr;
    int64_t residue_limit = 0;
    int8_t mt[kPairsCodes * 32] = {};   // the compact matrix, transposed: mt[q][d] = M[d][q], padding row zero
};
void ends_route(EndsRouting& T, size_t n);

}  // namespace ssa
