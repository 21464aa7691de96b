// pairs.h -- the batch pair scorer's device interface (pairs.hip) and the
// layout pairs.cpp packs for it.  Independent of kernels.h: the search
// kernels and their source hash are not touched by this feature.
//
// One wave scores one GROUP of 64 pairs, one pair per lane, in int32.  The
// query runs down the rows (strips of kPairsRows rows held in VGPRs), the
// target's residues are streamed as columns, 4 per dword.  Everything a wave
// loads is lane-interleaved, so each load is one coalesced 256- or 512-byte
// row:
//   tres  [group][col / 4][lane]  uint32: 4 target codes, padded with kPairsPad
//   qres  [group][row / 4][lane]  uint32: 4 query codes, padded with kPairsPad
//   bnd   [group][col][lane]      int2 (H, F) of the strip's bottom row
//   lens  [group][lane]           uint2 (qlen, dlen); (0, 0): lane unused
//   out   [group][lane]           int32 score
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace ssa {

constexpr int kPairsRows = 8;        // strip height R: one ds_read_b64 per column holds a lane's R scores
constexpr uint32_t kPairsPad = 32;   // padding code (rows and columns): scores 0 against everything
constexpr int kPairsCodes = 33;      // residue codes 0..31 + the padding code

struct PairsGroup {
    uint32_t t_row;      // first 64-lane dword row of the group in tres
    uint32_t q_row;      // the same in qres
    uint32_t b_row;      // first 64-lane int2 row of the group in bnd
    uint32_t ncb;        // column blocks of 4 (>= 1)
    uint32_t nstrips;    // strips of kPairsRows rows (>= 1)
};

struct PairsArgs {
    const uint32_t* tres;
    const uint32_t* qres;
    int2* bnd;
    const PairsGroup* groups;
    const uint2* lens;
    int32_t* out;
    const int8_t* mt;    // [kPairsCodes][32]: mt[q * 32 + d] = M[d][q]; row kPairsPad all zero
    int32_t gap_open, gap_extend;
    uint32_t ngroups;
};

// LDS of one wave (= one workgroup): the per-lane strip profile and the matrix
constexpr size_t kPairsLds = (size_t)kPairsCodes * 64 * kPairsRows + (size_t)kPairsCodes * 32;

hipError_t launch_pairs(int algo, const PairsArgs& a, hipStream_t st);

}  // namespace ssa
