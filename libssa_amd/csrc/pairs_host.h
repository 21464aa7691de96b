// pairs_host.h -- host-side helpers the batch aligner (pairs_align.cpp) and
// the ends-free pair calls (pairs_ends.cpp) share: device buffers that only
// grow, and the walk's runs as CIGAR text.  Host code only (engine.h).
#pragma once
#include "engine.h"
#include "pairs_align.h"

namespace ssa {

constexpr size_t kPairsAlign = 256;
inline size_t pairs_align_up(size_t x) { return (x + kPairsAlign - 1) / kPairsAlign * kPairsAlign; }

// A device buffer and (optionally) its pinned host twin; kept between calls, only ever grows.
struct PairsBuf {
    uint8_t* d = nullptr;
    uint8_t* h = nullptr;
    size_t cap = 0;
    void need(size_t bytes, bool host, const char* what) {
        if (cap >= bytes && d) return;
        release();
        cap = bytes + bytes / 4 + kPairsAlign;
        check(hipMalloc((void**)&d, cap), what);
        if (host) check(hipHostMalloc((void**)&h, cap, hipHostMallocDefault), what);
    }
    void release() {
        if (d) (void)hipFree(d);
        if (h) (void)hipHostFree(h);
        d = h = nullptr;
        cap = 0;
    }
};

// runs (count << 2 | op) in traceback order -> "<count><op>" from the alignment's begin, a count of 1 omitted
inline uint32_t format_runs(const uint32_t* runs, uint32_t n, char* text) {
    static const char ops[4] = {'M', 'I', 'D', '?'};
    char* p = text;
    for (uint32_t r = n; r-- > 0;) {
        uint32_t cnt = runs[r] >> 2;
        if (cnt > 1) {
            char tmp[12];
            int k = 0;
            for (; cnt; cnt /= 10) tmp[k++] = (char)('0' + cnt % 10);
            while (k) *p++ = tmp[--k];
        }
        *p++ = ops[runs[r] & 3];
    }
    *p = 0;
    return (uint32_t)(p - text);
}

}  // namespace ssa
