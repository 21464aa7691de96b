// pairs_banded_host.h -- the host side of the banded pair calls that the local
// pair calls share (defined in pairs_banded.cpp; used by pairs_local.cpp, pairs_summary.cpp, pairs_xdrop.cpp and
// hits_summary.cpp): the
// band's clamp and validity rule, the batch ordered by shape and band with its
// BandStrip ranges, the chunk packer and the device buffers it fills.  Host
// code only.
#pragma once
#include <vector>

#include "hits_gather.h"
#include "pairs_banded.h"
#include "pairs_host.h"
#include "pairs_summary.h"

namespace ssa {

// Band values beyond [-qlen - 1, dlen + 1] are equivalent to the clamped ones.
int64_t clamp_band(int64_t k, uint64_t ql, uint64_t dl);
// The header's rule: an interval that meets the start and the end diagonals of the mask.
bool band_valid(int ends, int64_t m, int64_t n, int64_t lo, int64_t hi);

constexpr size_t kBandScoreChunkBudget = (size_t)256 << 20;   // ssa_amd_score_pairs'
constexpr size_t kBandAlignChunkBudget = (size_t)2 << 30;     // ssa_amd_align_pairs_ends'
constexpr size_t kBandPairDirBudget = (size_t)512 << 20;      // direction bits of one pair alone
constexpr size_t kBandDirRowBytes = 1024;                     // one 64-lane uint4 row of direction bits

// The buffers of the banded and the local calls (one call runs at a time), kept between calls.
struct BandedDevice {
    int device = -1;
    hipEvent_t ev[4] = {};
    bool events = false;
    PairsBuf up, bnd, dir, runs, out;
    PairsBuf stop;                      // the local calls' STOP bits (pairs_local.h)
};
BandedDevice& banded_device();
void banded_prepare_device(int dev_id);
// milliseconds between the events e and e + 1
double banded_elapsed(int e);

// 64-lane rows of direction bits a pair needs when it is alone in its group (an upper bound)
uint64_t pair_dir_rows(uint64_t ql, uint64_t dl, int64_t lo, int64_t hi);

// The device pairs of a call, ordered by shape and band and cut into groups of 64.
struct BandBatch {
    const uint8_t* qc;
    const uint64_t* qoff;
    const uint8_t* dc;
    const uint64_t* doff;
    const int64_t* lo;                  // clamped, by input index
    const int64_t* hi;
    std::vector<uint32_t> idx;          // by input index
    std::vector<BandGroup> groups;
    std::vector<BandStrip> strips;      // all groups'; BandGroup::s_row is global until a chunk is cut
    std::vector<uint64_t> drows;        // direction rows of each group
    std::vector<size_t> gbytes;         // device bytes of each group

    uint32_t qlen(size_t i) const { return (uint32_t)(qoff[i + 1] - qoff[i]); }
    uint32_t dlen(size_t i) const { return (uint32_t)(doff[i + 1] - doff[i]); }
    uint32_t nstrips(size_t i) const { return (qlen(i) + kPairsRows - 1) / kPairsRows; }

    // Orders the pairs (strip count, then lo, then hi), cuts the groups and their strips' ranges; row_bytes:
    // what the align call keeps per 64-lane row of a swept block.  Returns the cells the waves walk.
    uint64_t order(bool align, size_t row_bytes = kBandDirRowBytes);
};

// The same batch for pairs whose residues are not on the host (hits_summary.cpp): the length source is one
// descriptor per pair, which is also what a chunk uploads for the pair's lane.  order() is BandBatch's, and
// so are the groups, the strips and the chunks cut from them.
struct BandDescBatch {
    const HitDesc* desc;                // by input index
    const int64_t* lo;                  // clamped, by input index
    const int64_t* hi;
    std::vector<uint32_t> idx;
    std::vector<BandGroup> groups;
    std::vector<BandStrip> strips;
    std::vector<uint64_t> drows;
    std::vector<size_t> gbytes;

    uint32_t qlen(size_t i) const { return desc[i].qlen; }
    uint32_t dlen(size_t i) const { return desc[i].dlen; }
    uint32_t nstrips(size_t i) const { return (qlen(i) + kPairsRows - 1) / kPairsRows; }
    uint64_t order(bool align, size_t row_bytes = kBandDirRowBytes);
};

// One chunk: groups [g0, g1) laid out in the upload block, packed and uploaded.
struct BandChunk {
    size_t g0, g1, ng, nl, p0, p1;
    uint64_t drow = 0;                  // the align call: 64-lane rows of direction bits
    uint64_t nruns = 0;                 //   and run slots
    AlignLane* lanes = nullptr;         //   the host copy of the lanes
    uint64_t qrow = 0, trow = 0;        // 64-lane dword rows of qres and tres
    size_t up_bytes = 0;                // bytes of the upload block
    const HitDesc* desc = nullptr;      // banded_pack_chunk_tables: the lanes' descriptors on the device
    BandedArgs A{};
};

// Cuts the chunk that starts at g0 (within the byte budget, at least one
// group), packs it lane-interleaved into the pinned block and enqueues its
// upload; sizes every device buffer banded_kernel and banded_walk_kernel touch.
BandChunk banded_pack_chunk(BandBatch& B, size_t g0, bool align, int ends, const EndsRouting& T);
// The score call's chunk without the residue rows and the lens: the upload block holds the matrix, the
// groups, the strips, the bands and one descriptor per lane (K.desc); A.lens, A.qres and A.tres are left
// NULL for the caller, whose device-side packer writes K.nl lens, K.qrow and K.trow rows.
BandChunk banded_pack_chunk_tables(BandDescBatch& B, size_t g0, int ends, const EndsRouting& T);

// ------------------------------------ what the summary call shares (pairs_summary.cpp)
// One pair through the host align routine of the banded calls (pairs_banded.cpp; ends: the mask) or of the
// local calls (pairs_local.cpp; mode: canonical, with a local bit), a clamped valid band, scratch of the
// call's own; text: qlen + dlen + 1 bytes.  local_host_align returns true for the empty alignment of two
// non-empty sides.
void banded_host_align(int ends, const uint8_t* q, size_t ql, const uint8_t* d, size_t dl, int64_t lo, int64_t hi,
                       ssa_amd_pair_alignment_t& o, char* text);
bool local_host_align(int mode, const uint8_t* q, size_t ql, const uint8_t* d, size_t dl, int64_t lo, int64_t hi,
                      ssa_amd_pair_alignment_t& o, char* text);
// the local calls' canonical mode, and their band check (NULL bands: the full range of every pair)
int local_canonical(int mode);
bool local_bands_ok(int mode, const int64_t* band_lo, const int64_t* band_hi, const uint64_t* qoff,
                    const uint64_t* doff, size_t n, std::vector<int64_t>& lo, std::vector<int64_t>& hi);

// ------------------------------------ what the X-drop calls share (pairs_xdrop.cpp)
// pairs_local.cpp: its host routines with the row rule of DESIGN.md §9.8 (mode: canonical, a local end without
// a local begin; xdrop >= 0; both sides non-empty or not); dropped is set where the pair met a drop row.
int64_t xdrop_host_score(int mode, const uint8_t* q, size_t ql, const uint8_t* d, size_t dl, int64_t lo, int64_t hi,
                         int64_t xdrop, bool& dropped);
bool xdrop_host_align(int mode, const uint8_t* q, size_t ql, const uint8_t* d, size_t dl, int64_t lo, int64_t hi,
                      int64_t xdrop, ssa_amd_pair_alignment_t& o, char* text, bool& dropped);
// pairs_summary.cpp: the chunk's summary buffers (SummaryArgs over K.A; *h_sum: the pinned twin of sum)
SummaryArgs summary_chunk_args(const BandBatch& B, const BandChunk& K, int dev_id, const uint2** h_sum);
SummaryArgs summary_chunk_args(const std::vector<BandGroup>& groups, const BandChunk& K, int dev_id,
                               const uint2** h_sum);
// ... one device lane's record from its end cell and its words; true for the empty alignment under a local bit
bool summary_record(bool local, int2 end, uint2 words, ssa_amd_pair_summary_t& o);
// ... columns, matched and identical of a CIGAR text walked from (region[0], region[2]), added to o
void summary_count_text(const char* text, const uint8_t* q, const uint8_t* d, ssa_amd_pair_summary_t& o);

}  // namespace ssa
