// profile_host.h -- the profile (position-specific scoring matrix) recurrences
// on the host: the definition ssa_amd_profile_score_host computes and the
// device results are compared against.  Plain C++, no device and no library
// state, so a stand-alone program can include it.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

namespace ssa {

constexpr int64_t kProfileMin = -32768, kProfileMax = 32767;   // the range of a profile value

// every value of rows x 32 scores within the range
inline bool profile_values_ok(const int32_t* scores, size_t rows) {
    for (size_t i = 0; i < rows * 32; i++)
        if (scores[i] < kProfileMin || scores[i] > kProfileMax) return false;
    return true;
}

// offsets ascending and every code below 32
inline bool profile_targets_ok(const uint8_t* d_codes, const uint64_t* d_off, size_t n) {
    for (size_t e = 0; e < n; e++)
        if (d_off[e + 1] < d_off[e]) return false;
    for (uint64_t x = n ? d_off[0] : 0; n && x < d_off[n]; x++)
        if (d_codes[x] >= 32) return false;
    return true;
}

// pairs.cpp host_sw / host_nw (the reference's smith_waterman_64.c /
// needleman_wunsch_64.c) with M[d_j][q_i] replaced by prof[i * 32 + d_j];
// columns = DB sequence, rows = profile positions, he = 2 * rows scratch words
inline int64_t profile_sw(const uint8_t* d, size_t dn, const int32_t* prof, size_t rows, int64_t Q, int64_t R,
                          int64_t* he) {
    int64_t best = 0;
    std::fill(he, he + 2 * rows, 0);
    for (size_t j = 0; j < dn; j++) {
        const int32_t* col = prof + d[j];
        int64_t h = 0, f = 0;
        for (size_t i = 0; i < rows; i++) {
            const int64_t left = he[2 * i];
            const int64_t e = he[2 * i + 1];
            h = std::max<int64_t>(std::max(h + col[i * 32], std::max(e, f)), 0);
            best = std::max(best, h);
            he[2 * i] = h;
            const int64_t open = h + Q + R;
            he[2 * i + 1] = std::max(e + R, open);
            f = std::max(f + R, open);
            h = left;
        }
    }
    return best;
}

inline int64_t profile_nw(const uint8_t* d, size_t dn, const int32_t* prof, size_t rows, int64_t Q, int64_t R,
                          int64_t* he) {
    // an empty sequence: the recurrence's own boundary, one gap over the rows
    if (dn == 0) return rows == 0 ? 0 : Q + (int64_t)rows * R;
    for (size_t i = 0; i < rows; i++) {
        he[2 * i] = Q + (int64_t)(i + 1) * R;
        he[2 * i + 1] = 2 * Q + (int64_t)(i + 2) * R;
    }
    for (size_t j = 0; j < dn; j++) {
        const int32_t* col = prof + d[j];
        int64_t f = 2 * Q + (int64_t)(j + 2) * R;
        int64_t h = j == 0 ? 0 : Q + (int64_t)j * R;
        for (size_t i = 0; i < rows; i++) {
            const int64_t left = he[2 * i];
            const int64_t e = he[2 * i + 1];
            h = std::max(h + col[i * 32], std::max(e, f));
            he[2 * i] = h;
            const int64_t open = h + Q + R;
            he[2 * i + 1] = std::max(e + R, open);
            f = std::max(f + R, open);
            h = left;
        }
    }
    return he[2 * rows - 2];
}

}  // namespace ssa
