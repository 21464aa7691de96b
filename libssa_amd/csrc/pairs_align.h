// pairs_align.h -- the batch aligner's device interface (pairs_align.hip) and
// the host helpers it shares with the batch scorer (pairs.cpp).  The packing
// is pairs.h's: groups of 64 pairs, one pair per lane, everything a wave
// touches lane-interleaved.  On top of pairs.h's buffers:
//   fin   [group][query row][lane]        int2 (H, E) after the lane's last column (pass 1 -> 2)
//   dir   [group][strip][col / 4][lane]   uint2: 4 columns x 8 rows x 2 bits (pass 3 -> 4);
//                                         column k of the block at bits 16k.., row r at 2r: bit 0 LEFT, bit 1 UP
//   runs  [lane's slot .. + cap)          uint32 count << 2 | op, in traceback order (pass 4)
#pragma once
#include <algorithm>
#include <atomic>
#include <cstring>
#include <thread>
#include <vector>

#include "common.h"
#include "pairs.h"

namespace ssa {

// positions travel as col << 16 | row; 0xffff in the column half means "none"
constexpr uint32_t kAlignMaxLen = 65535;          // both lengths below this go to the device
constexpr uint32_t kAlignNoPos = 0xffff0000u;     // any position >= this: no cell

constexpr uint32_t kOpM = 0, kOpI = 1, kOpD = 2;

struct AlignGroup {
    uint32_t t_row, q_row, b_row;   // as PairsGroup; the group's fin rows start at q_row * 4
    uint32_t ncb, nstrips;          // the extents this pass sweeps (0: nothing to do)
    uint32_t d_row;                 // first 64-lane uint2 row of the group in dir
};

struct AlignLane {       // per lane, passes 2 and 4
    uint32_t a_end, b_end;          // the end cell (query row, target column)
    uint32_t a_begin, b_begin;      // pass 4: where the walk stops
    int32_t best;                   // pass 2: the score to reach
    uint32_t used;                  // 0: the lane has no pair in this pass
    uint32_t slot, cap;             // pass 4: the lane's run slot in runs and its size
};

struct AlignArgs {
    const uint32_t* tres;
    const uint32_t* qres;
    int2* bnd;
    const AlignGroup* groups;
    const uint2* lens;              // (qlen, dlen) per lane; (0, 0): unused
    const AlignLane* lanes;
    const int8_t* mt;               // as PairsArgs::mt
    int2* fin;
    uint2* dir;
    uint32_t* runs;
    int2* out;                      // pass 1: (best, pos); pass 2: (pos, 0); pass 3: (NW score, 0); pass 4: (runs, 0)
    int32_t gap_open, gap_extend;
    uint32_t ngroups;
};

// pass: 0 forward (SW), 1 reverse (SW), 2 directions (nw selects the boundaries), 3 walk
hipError_t launch_pairs_align(int pass, bool nw, const AlignArgs& a, hipStream_t st);

// ------------------------------------------------ shared with pairs.cpp
// fn(begin, end) over [0, n) in ranges of `grain` items that the workers take
// from a shared counter (the items are sorted by size, so equal contiguous
// shares would not be equal work).  set_thread_count gives the worker count;
// by default the machine's cores, at most 16.
template <class F>
void parallel_ranges(size_t n, size_t grain, F fn) {
    grain = std::max<size_t>(grain, 1);
    size_t workers = cfg().thread_count ? cfg().thread_count
                                        : std::min<size_t>(16, std::max(1u, std::thread::hardware_concurrency()));
    workers = std::max<size_t>(1, std::min(workers, (n + grain - 1) / grain));
    std::atomic<size_t> next{0};
    auto work = [&]() {
        for (size_t b; (b = next.fetch_add(grain)) < n;) fn(b, std::min(n, b + grain));
    };
    std::vector<std::thread> pool;
    for (size_t w = 1; w < workers; w++) pool.emplace_back(work);
    work();
    for (auto& t : pool) t.join();
}

// One lane's codes into its column of a lane-interleaved block: 4 codes per
// dword, consecutive dwords 256 B apart (dst = the lane's first dword; the
// block is already filled with the padding code).
inline void interleave(uint8_t* dst, const uint8_t* src, uint32_t n) {
    uint32_t i = 0;
    for (; i + 4 <= n; i += 4) memcpy(dst + (size_t)(i / 4) * 256, src + i, 4);
    for (; i < n; i++) dst[(size_t)(i / 4) * 256 + (i & 3)] = src[i];
}

// pairs.cpp: the reference's 64-bit recurrences (he = 2 * qn scratch words)
int64_t host_sw(const uint8_t* d, size_t dn, const uint8_t* q, size_t qn, const int64_t* M, int64_t Q, int64_t R,
                int64_t* he);
int64_t host_nw(const uint8_t* d, size_t dn, const uint8_t* q, size_t qn, const int64_t* M, int64_t Q, int64_t R,
                int64_t* he);
// pairs.cpp: the device of this call made current and the pair calls' stream;
// false when no HIP device is visible
bool pairs_use_device(int* device, hipStream_t* stream);

}  // namespace ssa
