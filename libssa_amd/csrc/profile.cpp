// profile.cpp -- position-specific scoring matrices (ssa_amd_profile_*): the
// profile object and the exact host path.  The searches are api.cpp's.
#include <new>
#include <vector>

#include "common.h"
#include "pairs_align.h"   // parallel_ranges
#include "profile_host.h"

namespace ssa {

int profile_score_host(const ssa_amd_profile* p, int algo, const uint8_t* d_codes, const uint64_t* d_off, size_t n,
                       int64_t* scores) {
    if (algo != SSA_AMD_SW && algo != SSA_AMD_NW) return 1;
    if (n == 0) return 0;
    if (!p || !d_codes || !d_off || !scores) return 1;
    if (!profile_targets_ok(d_codes, d_off, n)) return 1;
    const bool nw = algo == SSA_AMD_NW;
    const int64_t Q = cfg().gap_open, R = cfg().gap_extend;
    const size_t rows = p->nrows;
    const int32_t* prof = p->rows.data();
    parallel_ranges(n, 8, [&](size_t b, size_t e) {
        std::vector<int64_t> he(2 * rows);
        for (size_t k = b; k < e; k++) {
            const uint8_t* d = d_codes + d_off[k];
            const size_t dn = (size_t)(d_off[k + 1] - d_off[k]);
            scores[k] = nw ? profile_nw(d, dn, prof, rows, Q, R, he.data()) : profile_sw(d, dn, prof, rows, Q, R, he.data());
        }
    });
    return 0;
}

}  // namespace ssa

using namespace ssa;

extern "C" {

p_ssa_profile ssa_amd_profile_create(const int32_t* scores, size_t rows) {
    if (!scores || rows == 0 || !profile_values_ok(scores, rows)) return nullptr;
    ssa_amd_profile* p = new (std::nothrow) ssa_amd_profile();
    if (!p) return nullptr;
    p->rows.assign(scores, scores + rows * 32);
    p->nrows = rows;
    return p;
}

p_ssa_profile ssa_amd_profile_from_query(p_query query, size_t view) {
    if (!query) return nullptr;
    const std::vector<QueryView> v = query_views(query);
    if (view >= v.size() || v[view].len == 0) return nullptr;
    const int64_t* M = matrix().m;
    std::vector<int32_t> rows(v[view].len * 32);
    for (size_t i = 0; i < v[view].len; i++)
        for (int c = 0; c < 32; c++) {
            const int64_t x = M[((size_t)c << 5) + v[view].seq[i]];
            if (x < kProfileMin || x > kProfileMax) return nullptr;
            rows[i * 32 + c] = (int32_t)x;
        }
    return ssa_amd_profile_create(rows.data(), v[view].len);
}

size_t ssa_amd_profile_rows(p_ssa_profile p) { return p ? p->nrows : 0; }

void ssa_amd_profile_free(p_ssa_profile p) { delete p; }

int ssa_amd_profile_score_host(p_ssa_profile p, int algo, const uint8_t* d_codes, const uint64_t* d_off, size_t n,
                               int64_t* scores) {
    return profile_score_host(p, algo, d_codes, d_off, n, scores);
}

}  // extern "C"
