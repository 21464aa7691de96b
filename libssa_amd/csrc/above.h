// above.h -- the select kernel of the threshold search (ssa_amd_search_above;
// above.hip).  After the DP kernels have written the int32
// score of every (view, entry), above_select forwards the entries at or above
// a fixed threshold to the host -- where the top-k search runs the candidate
// filter of kernels.h.  A threshold has no insertion order: no order array,
// no bounds, no dependency between blocks.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace ssa {

constexpr uint32_t kAbovePer = 4;                     // consecutive scores per thread: one 16-byte load
constexpr uint32_t kAboveThreads = 256;
constexpr uint32_t kAboveBlock = kAbovePer * kAboveThreads;   // entries one block covers

struct AboveArgs {
    const int32_t* scores;     // [n] view-major (view * entries + entry), 16-byte aligned;
                               // INT32_MIN = overflowed (exact value from the re-score tier)
    uint32_t n;
    int32_t t32;               // an entry is forwarded iff score == INT32_MIN || score >= t32
    const uint32_t* ovf_count; // view v's overflowed lanes at ovf_count[v * ovf_stride] ...
    uint32_t ovf_stride, nviews;
    uint32_t* counters;        // kernels.h FilterArgs::counters, zero on entry: [0] forwarded entries
                               // (one atomicAdd per block), [2] *status, [3 + v] view v's count
    const uint32_t* status;    // the pair launch's strip-part wait status word; null: none
    uint2* cand;               // [n] (position, score), in position order inside a block's range
};

// the device threshold of a 64-bit one: a superset (the host re-checks the
// exact score), and never INT32_MIN, which marks the overflowed lanes
inline int32_t above_t32(int64_t min_score) {
    return (int32_t)(min_score < (int64_t)INT32_MIN + 1 ? (int64_t)INT32_MIN + 1
                     : min_score > (int64_t)INT32_MAX   ? (int64_t)INT32_MAX
                                                        : min_score);
}

hipError_t launch_above(const AboveArgs& a, hipStream_t st);

}  // namespace ssa
