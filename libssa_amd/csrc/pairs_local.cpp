// pairs_local.cpp -- ssa_amd_score_pairs_local / ssa_amd_align_pairs_local:
// the banded ends-free family (pairs_banded.cpp) with a local
// begin and / or a local end.  A local begin floors H at 0 in
// every existing cell and lets the walk stop where max(D, E, F) <= 0; a local
// end takes its end cell among all existing real cells, the smallest
// (d_end, q_end) of the greatest H.  Mode 63 is Smith-Waterman in a band, 42
// and 21 extend from a fixed begin / towards a fixed end.  A canonical mode
// below 16 is the banded call's (with bands) or the ends call's (without).
// Packing, ordering and chunking are pairs_banded.cpp's, through
// pairs_banded_host.h; a NULL band is the full range of every pair.  A chunk of
// the score call runs local_kernel<false>; a chunk of the align call the end
// pass (under a local end), the direction pass and the walk back to back, one
// synchronisation per chunk.  What the device does not take goes through the
// int64 routine below, which keeps its matrices for the band only.
#include <algorithm>
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "pairs_banded_host.h"
#include "pairs_local.h"

namespace ssa {

namespace {

// A local begin frees both begins, a local end both ends.
int canonical(int mode) {
    if (mode & kLocalBegin) mode |= kFreeQBegin | kFreeDBegin;
    if (mode & kLocalEnd) mode |= kFreeQEnd | kFreeDEnd;
    return mode;
}

// ------------------------------------------------------------ the host path
constexpr int64_t kNeg = INT64_MIN / 4;     // minus infinity: room for every sum that starts from it

struct HostScratch {
    std::vector<int64_t> h, f;      // band width + 1 words each
    std::vector<uint8_t> dir;       // rows x band width
    std::vector<uint32_t> runs;
};

// One pair, both sides non-empty, a valid clamped band, a canonical mode with a
// local bit: pairs_banded.cpp's host_banded (the same row layout of h, f and
// dir) with the floor and kDirStop under a local begin and, under a local end,
// the candidates of all existing real cells with a finite H -- greater, or
// equal and the smaller (j, i).  The score is the end cell's H as it stands;
// the caller takes max(0, score).  xdrop >= 0 (a local end without a local
// begin): the candidates are cut row by row -- a row keeps its
// greatest finite H and the smallest column that attains it; best starts at 0
// with no end cell; a row whose maximum lies more than xdrop below best is the
// drop row, the loop stops there and *dropped is set; else a greater maximum,
// or an equal one in a smaller column than the end cell's, moves the end cell.
EndCell host_local(int mode, const uint8_t* q, size_t qn, const uint8_t* d, size_t dn, int64_t lo, int64_t hi,
                   const int64_t* M, int64_t Q, int64_t R, int64_t* h, int64_t* f, uint8_t* dir, int64_t xdrop = -1,
                   bool* dropped = nullptr) {
    const bool fqb = mode & kFreeQBegin, fqe = mode & kFreeQEnd, fdb = mode & kFreeDBegin, fde = mode & kFreeDEnd;
    const bool lb = mode & kLocalBegin, le = mode & kLocalEnd;
    const int64_t m = (int64_t)qn, n = (int64_t)dn, W = hi - lo + 1, goe = Q + R;
    auto in_band = [&](int64_t k) { return k >= lo && k <= hi; };
    const bool zero = in_band(0);
    auto col_m1 = [&](int64_t i) -> int64_t {            // H(i, -1), i >= -1
        if (!in_band(-1 - i)) return kNeg;
        if (i < 0 || fqb) return 0;
        return zero ? Q + (i + 1) * R : kNeg;
    };
    auto row_m1 = [&](int64_t j) -> int64_t {            // H(-1, j), j >= 0
        if (!in_band(j + 1)) return kNeg;
        if (fdb) return 0;
        return zero ? Q + (j + 1) * R : kNeg;
    };
    // ---- row -1: k = j + 1 - lo
    for (int64_t k = 0; k <= W; k++) h[k] = f[k] = kNeg;
    for (int64_t j = std::max<int64_t>(-1, lo - 1); j <= std::min(n - 1, hi - 1); j++) {
        const int64_t v = j < 0 ? col_m1(-1) : row_m1(j);
        h[j + 1 - lo] = v;
        f[j + 1 - lo] = (j >= 0 && v > kNeg / 2) ? v + goe : kNeg;
    }
    int64_t row_best = INT64_MIN, col_best = INT64_MIN, best = xdrop >= 0 ? 0 : INT64_MIN;
    size_t row_col = 0, col_row = 0;
    int64_t best_i = 0, best_j = 0;
    bool have = false;                                   // under xdrop: an end cell exists
    for (int64_t i = 0; i < m; i++) {
        int64_t row_m = kNeg, row_c = 0;                 // under xdrop: the row's greatest finite H, its first column
        const int64_t* srow = M + q[i];                  // M[d][q[i]] = srow[d << 5]
        const int64_t j1 = std::min(n - 1, i + hi);
        int64_t j = std::max<int64_t>(-1, i + lo);
        int64_t e = kNeg;                                // E entering (i, j): nothing left of the band
        if (j == -1) {
            if (i + hi >= -1) {                          // column -1 is in the row's band
                const int64_t v = col_m1(i);
                h[-1 - i - lo] = v;
                f[-1 - i - lo] = kNeg;
                if (v > kNeg / 2) e = v + goe;
            }
            j = 0;
        }
        uint8_t* drow = dir ? dir + (size_t)i * (size_t)W : nullptr;
        for (; j <= j1; j++) {
            const int64_t k = j - i - lo;
            const int64_t diag = h[k] + srow[(size_t)d[j] << 5];
            const int64_t fv = f[k + 1];
            const int64_t mx = std::max(diag, fv);
            const int64_t raw = std::max(mx, e);
            const int64_t hv = lb ? std::max<int64_t>(raw, 0) : raw;
            h[k] = hv;
            const int64_t t = hv + goe, e2 = e + R, f2 = fv + R;
            if (drow)
                drow[k] = (uint8_t)((e > mx ? kDirLeft : 0) | (fv > diag ? kDirUp : 0) | (e2 > t ? kDirExtLeft : 0) |
                                    (f2 > t ? kDirExtUp : 0) | (lb && raw <= 0 ? kDirStop : 0));
            e = std::max(e2, t);
            f[k] = std::max(f2, t);
            if (le) {
                if (xdrop >= 0) {
                    if (hv > kNeg / 2 && hv > row_m) row_m = hv, row_c = j;
                    continue;
                }
                // rows ascend: an equal cell wins only from a smaller column
                if (hv > kNeg / 2 && (hv > best || (hv == best && j < best_j))) {
                    best = hv;
                    best_i = i;
                    best_j = j;
                }
                continue;
            }
            // candidates by ascending position, each replacing the kept one when >=
            if (i == m - 1 && (fde || j == n - 1) && hv >= row_best) {
                row_best = hv;
                row_col = (size_t)j;
            }
            if (fqe && j == n - 1 && hv >= col_best) {
                col_best = hv;
                col_row = (size_t)i;
            }
        }
        if (xdrop >= 0 && row_m > kNeg / 2) {
            if (best - row_m > xdrop) {
                if (dropped) *dropped = true;
                break;
            }
            if (row_m > best || (row_m == best && have && row_c < best_j)) {
                best = row_m;
                best_i = i;
                best_j = row_c;
                have = true;
            }
        }
    }
    if (le) return EndCell{best, (size_t)best_i, (size_t)best_j};
    return ends_pick_cell(row_best, row_col, col_best, col_row, qn, dn);
}

// The walk (next_op, and under a local begin the STOP test at a cell it stands
// on through its H) from the end cell until it stops or leaves the matrix;
// false if it ever stands outside the band.
bool host_walk(const uint8_t* dir, int64_t lo, int64_t W, const EndCell& c, std::vector<uint32_t>& runs) {
    runs.clear();
    int64_t i = (int64_t)c.q_end, j = (int64_t)c.d_end;
    uint32_t op = kOpM;
    while (i >= 0 && j >= 0) {
        const int64_t k = j - i - lo;
        if (k < 0 || k >= W) return false;
        const uint32_t b = dir[(size_t)i * (size_t)W + (size_t)k];
        const bool in_gap = (op == kOpI && (b & kDirExtLeft)) || (op == kOpD && (b & kDirExtUp));
        if (!in_gap && (b & kDirStop)) break;
        op = next_op(op, b);
        if (!runs.empty() && (runs.back() & 3) == op) runs.back() += 4;
        else runs.push_back(1u << 2 | op);
        j -= op != kOpD;
        i -= op != kOpI;
    }
    return true;
}

// Region and text from the end cell and the walk's runs.  Under a local begin
// the walk stopped on, or left the matrix at, the cell (i, j) in front of the
// alignment: the begins are (i + 1, j + 1).  Else the ends calls' rule.
uint32_t finish_alignment(int mode, size_t q_end, size_t d_end, std::vector<uint32_t>& runs, uint64_t region[4],
                          char* text) {
    if (!(mode & kLocalBegin)) return ends_finish_alignment(mode & 15, q_end, d_end, runs, region, text);
    int64_t qc = 0, dc = 0;
    for (const uint32_t r : runs) {
        if ((r & 3) != kOpI) qc += r >> 2;
        if ((r & 3) != kOpD) dc += r >> 2;
    }
    region[0] = (uint64_t)((int64_t)q_end - qc + 1);
    region[1] = q_end;
    region[2] = (uint64_t)((int64_t)d_end - dc + 1);
    region[3] = d_end;
    return format_runs(runs.data(), (uint32_t)runs.size(), text);
}

// the empty alignment: score 0, region zeros, no text
void empty_alignment(ssa_amd_pair_alignment_t& o, char* text) {
    o.score = 0;
    for (auto& r : o.region) r = 0;
    o.cigar_len = 0;
    text[0] = 0;
}

int64_t host_score(int mode, const uint8_t* q, size_t ql, const uint8_t* d, size_t dl, int64_t lo, int64_t hi,
                   HostScratch& S, int64_t xdrop = -1, bool* dropped = nullptr) {
    if (ql == 0 || dl == 0) return 0;       // ends_empty_score of a canonical mode with a local bit
    const size_t W = (size_t)(hi - lo + 1);
    if (S.h.size() < W + 1) S.h.resize(W + 1), S.f.resize(W + 1);
    const EndCell c = host_local(mode, q, ql, d, dl, lo, hi, matrix().m, cfg().gap_open, cfg().gap_extend, S.h.data(),
                                 S.f.data(), nullptr, xdrop, dropped);
    return std::max<int64_t>(c.score, 0);
}

// returns true for the empty alignment of two non-empty sides
bool host_align(int mode, const uint8_t* q, size_t ql, const uint8_t* d, size_t dl, int64_t lo, int64_t hi,
                HostScratch& S, ssa_amd_pair_alignment_t& o, char* text, int64_t xdrop = -1, bool* dropped = nullptr) {
    o.flags = 1;
    if (ql == 0 || dl == 0) {
        empty_alignment(o, text);
        return false;
    }
    const size_t W = (size_t)(hi - lo + 1);
    if (S.h.size() < W + 1) S.h.resize(W + 1), S.f.resize(W + 1);
    if (S.dir.size() < ql * W) S.dir.resize(ql * W);
    const EndCell c = host_local(mode, q, ql, d, dl, lo, hi, matrix().m, cfg().gap_open, cfg().gap_extend, S.h.data(),
                                 S.f.data(), S.dir.data(), xdrop, dropped);
    if (c.score <= 0) {
        empty_alignment(o, text);
        return true;
    }
    if (!host_walk(S.dir.data(), lo, (int64_t)W, c, S.runs)) fatal("pairs_local: the walk left the band");
    o.score = c.score;
    o.cigar_len = finish_alignment(mode, c.q_end, c.d_end, S.runs, o.region, text);
    return false;
}

// ---------------------------------------------------------------- arguments
// Clamps every band into lo / hi (NULL bands: the full range); false for a pair
// of two non-empty sides whose band admits no alignment under the mode.
bool bands_ok(int mode, const int64_t* band_lo, const int64_t* band_hi, const uint64_t* qoff, const uint64_t* doff,
              size_t n, std::vector<int64_t>& lo, std::vector<int64_t>& hi) {
    lo.resize(n);
    hi.resize(n);
    for (size_t i = 0; i < n; i++) {
        const uint64_t ql = qoff[i + 1] - qoff[i], dl = doff[i + 1] - doff[i];
        lo[i] = band_lo ? clamp_band(band_lo[i], ql, dl) : -(int64_t)ql - 1;
        hi[i] = band_hi ? clamp_band(band_hi[i], ql, dl) : (int64_t)dl + 1;
        if (ql && dl && !band_valid(mode & 15, (int64_t)ql, (int64_t)dl, lo[i], hi[i])) return false;
    }
    return true;
}

// direction bits and, under a local begin, STOP bits of one 64-lane row of a swept block
size_t row_bytes(int mode) { return kBandDirRowBytes + ((mode & kLocalBegin) ? 256 : 0); }

LocalArgs local_args(const BandChunk& K, int mode, bool align) {
    LocalArgs A;
    A.b = K.A;
    A.stop = nullptr;
    if (align && (mode & kLocalBegin)) {
        BandedDevice& P = banded_device();
        P.stop.need(std::max<size_t>((size_t)K.drow, 1) * 256, false, "pairs_local stop bits");
        A.stop = (uint32_t*)P.stop.d;
    }
    return A;
}

}  // namespace

// ---- shared with pairs_summary.cpp (pairs_banded_host.h)
int local_canonical(int mode) { return canonical(mode); }

bool local_bands_ok(int mode, const int64_t* band_lo, const int64_t* band_hi, const uint64_t* qoff,
                    const uint64_t* doff, size_t n, std::vector<int64_t>& lo, std::vector<int64_t>& hi) {
    return bands_ok(mode, band_lo, band_hi, qoff, doff, n, lo, hi);
}

bool local_host_align(int mode, const uint8_t* q, size_t ql, const uint8_t* d, size_t dl, int64_t lo, int64_t hi,
                      ssa_amd_pair_alignment_t& o, char* text) {
    HostScratch S;
    return host_align(mode, q, ql, d, dl, lo, hi, S, o, text);
}

// ---- shared with pairs_xdrop.cpp (pairs_banded_host.h): the routines above with the row rule
int64_t xdrop_host_score(int mode, const uint8_t* q, size_t ql, const uint8_t* d, size_t dl, int64_t lo, int64_t hi,
                         int64_t xdrop, bool& dropped) {
    HostScratch S;
    return host_score(mode, q, ql, d, dl, lo, hi, S, xdrop, &dropped);
}

bool xdrop_host_align(int mode, const uint8_t* q, size_t ql, const uint8_t* d, size_t dl, int64_t lo, int64_t hi,
                      int64_t xdrop, ssa_amd_pair_alignment_t& o, char* text, bool& dropped) {
    HostScratch S;
    return host_align(mode, q, ql, d, dl, lo, hi, S, o, text, xdrop, &dropped);
}

int score_pairs_local(int mode, const int64_t* band_lo, const int64_t* band_hi, const uint8_t* qc,
                      const uint64_t* qoff, const uint8_t* dc, const uint64_t* doff, size_t n, int64_t* scores) {
    const double t0 = now_ms();
    if (mode < 0 || mode > 63 || !band_lo != !band_hi) return 1;
    mode = canonical(mode);
    if (mode < 16)
        return band_lo ? score_pairs_banded(mode, band_lo, band_hi, qc, qoff, dc, doff, n, scores)
                       : score_pairs_ends(mode, qc, qoff, dc, doff, n, scores);
    std::vector<int64_t> lo, hi;
    if (!ends_args_ok(mode & 15, qc, qoff, dc, doff, n) || (n && !scores)) return 1;
    if (!bands_ok(mode, band_lo, band_hi, qoff, doff, n, lo, hi)) return 1;
    ssa_amd_pairs_stats_t S{};
    S.strip_rows = kPairsRows;
    S.device = -1;
    if (n == 0) {
        set_pairs_stats(S);
        return 0;
    }
    if (!matrix().ready) fatal("Scoring matrix not initialized");
    EndsRouting T;
    ends_route(T, n);
    S.pairs = n;
    S.device = T.device ? T.dev_id : -1;
    snprintf(S.kernel, sizeof S.kernel, "pairs_local_i32");

    BandBatch B{qc, qoff, dc, doff, lo.data(), hi.data(), {}, {}, {}, {}, {}};
    std::vector<size_t> todo;        // the pairs of the host path
    for (size_t i = 0; i < n; i++) {
        const uint64_t ql = qoff[i + 1] - qoff[i], dl = doff[i + 1] - doff[i];
        S.cells += ql * dl;
        if (T.device && ql && dl && (int64_t)(ql + dl) <= T.residue_limit && ql + dl < ((uint64_t)1 << 31))
            B.idx.push_back((uint32_t)i);
        else
            todo.push_back(i);
    }
    // ---- the host path
    const double th0 = now_ms();
    S.host_pairs = todo.size();
    parallel_ranges(todo.size(), 8, [&](size_t b, size_t e) {
        HostScratch W;
        for (size_t k = b; k < e; k++) {
            const size_t i = todo[k];
            scores[i] = host_score(mode, qc + qoff[i], qoff[i + 1] - qoff[i], dc + doff[i], doff[i + 1] - doff[i],
                                   lo[i], hi[i], W);
        }
    });
    S.host_ms = now_ms() - th0;

    // ---- the device path
    if (!B.idx.empty()) {
        BandedDevice& P = banded_device();
        banded_prepare_device(T.dev_id);
        const double tp0 = now_ms();
        S.swept_cells = B.order(false);
        S.groups = (uint32_t)B.groups.size();
        S.pack_ms += now_ms() - tp0;
        for (size_t g0 = 0; g0 < B.groups.size();) {
            const double tc0 = now_ms();
            const BandChunk K = banded_pack_chunk(B, g0, false, mode & 15, T);
            const LocalArgs A = local_args(K, mode, false);
            S.pack_ms += now_ms() - tc0;
            check(hipEventRecord(P.ev[0], T.stream), "hipEventRecord");
            check(launch_pairs_local(0, mode, A, T.stream), "pairs_local_i32");
            check(hipEventRecord(P.ev[1], T.stream), "hipEventRecord");
            check(hipMemcpyAsync(P.out.h, P.out.d, K.nl * sizeof(int2), hipMemcpyDeviceToHost, T.stream),
                  "pairs_local scores copy");
            check(hipStreamSynchronize(T.stream), "pairs_local synchronize");
            S.kernel_ms += banded_elapsed(0);
            const int2* h_out = (const int2*)P.out.h;
            for (size_t p = K.p0; p < K.p1; p++) scores[B.idx[p]] = std::max(h_out[p - K.p0].x, 0);
            S.chunks++;
            S.launches++;
            g0 = K.g1;
        }
    }
    S.total_ms = now_ms() - t0;
    set_pairs_stats(S);
    return 0;
}

int align_pairs_local(int mode, const int64_t* band_lo, const int64_t* band_hi, const uint8_t* qc,
                      const uint64_t* qoff, const uint8_t* dc, const uint64_t* doff, size_t n,
                      ssa_amd_pair_alignment_t* out, char* cigars, size_t cigar_cap) {
    const double t0 = now_ms();
    if (mode < 0 || mode > 63 || !band_lo != !band_hi) return 1;
    mode = canonical(mode);
    if (mode < 16)
        return band_lo ? align_pairs_banded(mode, band_lo, band_hi, qc, qoff, dc, doff, n, out, cigars, cigar_cap)
                       : align_pairs_ends(mode, qc, qoff, dc, doff, n, out, cigars, cigar_cap);
    const bool le = mode & kLocalEnd;
    std::vector<int64_t> lo, hi;
    if (!ends_args_ok(mode & 15, qc, qoff, dc, doff, n) || (n && (!out || !cigars))) return 1;
    if (!bands_ok(mode, band_lo, band_hi, qoff, doff, n, lo, hi)) return 1;
    ssa_amd_align_pairs_stats_t S{};
    S.device = -1;
    if (n == 0) {
        set_align_pairs_stats(S);
        return 0;
    }
    if (!matrix().ready) fatal("Scoring matrix not initialized");
    // every pair's CIGAR slot: qlen + dlen + 1 bytes, in input order
    std::vector<uint64_t> coff(n + 1);
    coff[0] = 0;
    for (size_t i = 0; i < n; i++) coff[i + 1] = coff[i] + (qoff[i + 1] - qoff[i]) + (doff[i + 1] - doff[i]) + 1;
    if (cigar_cap < coff[n]) return 1;

    EndsRouting T;
    ends_route(T, n);
    S.pairs = n;
    S.device = T.device ? T.dev_id : -1;

    BandBatch B{qc, qoff, dc, doff, lo.data(), hi.data(), {}, {}, {}, {}, {}};
    std::vector<size_t> todo;        // the pairs of the host path
    for (size_t i = 0; i < n; i++) {
        const uint64_t ql = qoff[i + 1] - qoff[i], dl = doff[i + 1] - doff[i];
        S.cells += ql * dl;
        // the banded call's conditions; the 512 MiB of the pair include the STOP bits
        if (T.device && ql && dl && (int64_t)(ql + dl) <= T.residue_limit && ql < kAlignMaxLen && dl < kAlignMaxLen &&
            pair_dir_rows(ql, dl, lo[i], hi[i]) * row_bytes(mode) <= kBandPairDirBudget)
            B.idx.push_back((uint32_t)i);
        else
            todo.push_back(i);
    }
    std::atomic<uint64_t> zeros{0};
    auto on_host = [&](HostScratch& W, size_t i) {
        out[i].cigar_off = coff[i];
        if (host_align(mode, qc + qoff[i], qoff[i + 1] - qoff[i], dc + doff[i], doff[i + 1] - doff[i], lo[i], hi[i], W,
                       out[i], cigars + coff[i]))
            zeros++;
    };
    // ---- the host path
    const double th0 = now_ms();
    S.host_pairs = todo.size();
    parallel_ranges(todo.size(), 4, [&](size_t b, size_t e) {
        HostScratch W;
        for (size_t k = b; k < e; k++) on_host(W, todo[k]);
    });
    S.host_ms = now_ms() - th0;

    // ---- the device path
    if (!B.idx.empty()) {
        BandedDevice& P = banded_device();
        banded_prepare_device(T.dev_id);
        snprintf(S.kernels, sizeof S.kernels, le ? "pairs_local_end,pairs_local_dir,pairs_local_walk"
                                                  : "pairs_local_dir,pairs_local_walk");
        const double tp0 = now_ms();
        B.order(true, row_bytes(mode));
        S.groups = (uint32_t)B.groups.size();
        S.pack_ms += now_ms() - tp0;
        for (size_t g0 = 0; g0 < B.groups.size();) {
            const double tc0 = now_ms();
            const BandChunk K = banded_pack_chunk(B, g0, true, mode & 15, T);
            const LocalArgs A = local_args(K, mode, true);
            S.pack_ms += now_ms() - tc0;
            S.dir_bytes += K.drow * row_bytes(mode);
            // ---- the end cells (a local end), the directions, then the walk from out's end cells
            check(hipEventRecord(P.ev[0], T.stream), "hipEventRecord");
            if (le) check(launch_pairs_local(0, mode, A, T.stream), "pairs_local_end");
            check(hipEventRecord(P.ev[1], T.stream), "hipEventRecord");
            check(launch_pairs_local(1, mode, A, T.stream), "pairs_local_dir");
            check(hipEventRecord(P.ev[2], T.stream), "hipEventRecord");
            check(launch_pairs_local(2, mode, A, T.stream), "pairs_local_walk");
            check(hipEventRecord(P.ev[3], T.stream), "hipEventRecord");
            check(hipMemcpyAsync(P.out.h, P.out.d, K.nl * (sizeof(int2) + sizeof(uint32_t)), hipMemcpyDeviceToHost,
                                 T.stream),
                  "pairs_local results copy");
            if (K.nruns)
                check(hipMemcpyAsync(P.runs.h, P.runs.d, K.nruns * sizeof(uint32_t), hipMemcpyDeviceToHost, T.stream),
                      "pairs_local runs copy");
            check(hipStreamSynchronize(T.stream), "pairs_local synchronize");
            if (le) S.fwd_ms += banded_elapsed(0);
            S.dir_ms += banded_elapsed(1);
            S.walk_ms += banded_elapsed(2);
            S.launches += le ? 3 : 2;

            // ---- region and text
            const double tt0 = now_ms();
            const int2* h_out = (const int2*)P.out.h;
            const uint32_t* h_runs = (const uint32_t*)P.runs.h;
            const uint32_t* h_nruns = (const uint32_t*)(h_out + K.nl);
            std::atomic<uint64_t> lost{0};
            parallel_ranges(K.p1 - K.p0, 64, [&](size_t b, size_t e) {
                std::vector<uint32_t> runs;
                HostScratch W;
                for (size_t l = b; l < e; l++) {
                    const AlignLane& L = K.lanes[l];
                    const uint32_t i = B.idx[K.p0 + l];
                    if (h_nruns[l] == kBandWalkLost) {
                        // the walk stood outside what was stored (expected never): the host routine
                        lost++;
                        on_host(W, i);
                        continue;
                    }
                    ssa_amd_pair_alignment_t& o = out[i];
                    o.cigar_off = coff[i];
                    o.flags = 0;
                    if (h_out[l].x <= 0) {
                        empty_alignment(o, cigars + coff[i]);
                        zeros++;
                        continue;
                    }
                    o.score = h_out[l].x;
                    const uint32_t pos = (uint32_t)h_out[l].y;
                    const uint32_t nr = std::min(h_nruns[l], L.cap);
                    runs.assign(h_runs + L.slot, h_runs + L.slot + nr);
                    o.cigar_len = finish_alignment(mode, pos & 0xffff, pos >> 16, runs, o.region, cigars + coff[i]);
                }
            });
            S.device_fallbacks += lost.load();
            S.host_pairs += lost.load();
            S.text_ms += now_ms() - tt0;
            S.chunks++;
            g0 = K.g1;
        }
    }
    S.zero_pairs = zeros.load();
    S.kernel_ms = S.fwd_ms + S.dir_ms + S.walk_ms;
    S.total_ms = now_ms() - t0;
    set_align_pairs_stats(S);
    return 0;
}

}  // namespace ssa
