// pairs_xdrop.cpp -- ssa_amd_score_pairs_xdrop / ssa_amd_align_pairs_xdrop /
// ssa_amd_summarize_pairs_xdrop: the local pair calls of a mode with a local
// end and no local begin (canonical 42, 43, 46, 47) whose end candidates are
// cut at the first row that falls more than xdrop below the best score so far
// (DESIGN.md §9.8).  No cell is pruned: validation, ordering, chunking and
// packing are the local calls' (pairs_banded_host.h), and so are the
// direction pass, the walk and the summary sweep.  A chunk first runs the end
// pass (xdrop_kernel, pairs_xdrop.hip), whose result comes back at once: the
// score call counts the strips the waves entered; the align and the summary
// calls cut every group to the strip of its furthest end row, upload the group
// table again and run the existing kernels on what is left -- the walk only
// moves up and left, so nothing below an end row is ever read.  What the
// device does not take goes through pairs_local.cpp's int64 routine with the
// same row rule.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "pairs_banded_host.h"
#include "pairs_xdrop.h"

namespace ssa {

namespace {

// pairs of the last call that met a drop row, device and host pairs alike
std::atomic<uint64_t> g_dropped{0};

// the end pass's dropped flags and strip counts, kept between calls beside banded_device()'s buffers
struct XdropDevice {
    int device = -1;
    PairsBuf info;
} g_dev;

// 0 and the canonical mode, or non-zero: the local calls' checks, a negative xdrop, a mode that is not a local
// end from a begin that is not local
int check_mode(int& mode, int64_t xdrop, const int64_t* band_lo, const int64_t* band_hi) {
    if (mode < 0 || mode > 63 || xdrop < 0 || !band_lo != !band_hi) return 1;
    mode = local_canonical(mode);
    return ((mode & kLocalEnd) && !(mode & kLocalBegin)) ? 0 : 1;
}

// What the end pass left of a chunk, in pinned memory: valid until the next copy into the same buffers.
struct EndPass {
    const int2* out;            // (best, col << 16 | row) per lane
    const uint32_t* dropped;    // per lane
    const uint32_t* entered;    // per group
    double ms;
};

// Runs xdrop_kernel over the chunk between the events 0 and 1, copies its results back and waits for them.
EndPass end_pass(const BandChunk& K, int64_t xdrop, const EndsRouting& T) {
    BandedDevice& P = banded_device();
    XdropDevice& D = g_dev;
    if (D.device != T.dev_id) {
        D.info.release();
        D.device = T.dev_id;
    }
    const size_t info_bytes = (K.nl + K.ng) * sizeof(uint32_t);
    D.info.need(info_bytes, true, "pairs_xdrop flags");
    XdropArgs A;
    A.b = K.A;
    A.xdrop = (int32_t)std::min(xdrop, kXdropMax);
    A.dropped = (uint32_t*)D.info.d;
    A.entered = A.dropped + K.nl;
    check(hipEventRecord(P.ev[0], T.stream), "hipEventRecord");
    check(launch_pairs_xdrop(A, T.stream), "pairs_xdrop_end");
    check(hipEventRecord(P.ev[1], T.stream), "hipEventRecord");
    check(hipMemcpyAsync(P.out.h, P.out.d, K.nl * sizeof(int2), hipMemcpyDeviceToHost, T.stream),
          "pairs_xdrop end cells copy");
    check(hipMemcpyAsync(D.info.h, D.info.d, info_bytes, hipMemcpyDeviceToHost, T.stream), "pairs_xdrop flags copy");
    check(hipStreamSynchronize(T.stream), "pairs_xdrop synchronize");
    EndPass E;
    E.out = (const int2*)P.out.h;
    E.dropped = (const uint32_t*)D.info.h;
    E.entered = E.dropped + K.nl;
    E.ms = banded_elapsed(0);
    return E;
}

uint64_t count_dropped(const BandChunk& K, const EndPass& E) {
    uint64_t n = 0;
    for (size_t l = 0; l < K.p1 - K.p0; l++) n += E.dropped[l];
    return n;
}

// 64-lane rows of column blocks in the first `strips` strips of the batch's group g
uint64_t block_rows(const BandBatch& B, size_t g, uint32_t strips) {
    const BandStrip* S = B.strips.data() + B.groups[g].s_row;
    uint64_t rows = 0;
    for (uint32_t s = 0; s < strips; s++) rows += S[s].ncb;
    return rows;
}

// Cuts every group of the chunk to the strip of its furthest end row (a group without an end cell to no strip
// at all: its wave returns at once) and enqueues the upload of the group table; returns the rows of column
// blocks the later passes still sweep.  The strips' d_off are prefix sums, so the layout of dir stays.
uint64_t cut_groups(const BandBatch& B, const BandChunk& K, const EndPass& E, const EndsRouting& T) {
    BandedDevice& P = banded_device();
    BandGroup* hg = (BandGroup*)(P.up.h + ((const uint8_t*)K.A.groups - P.up.d));
    uint64_t rows = 0;
    for (size_t g = 0; g < K.ng; g++) {
        uint32_t cut = 0;
        for (size_t l = g * 64; l < std::min(g * 64 + 64, K.p1 - K.p0); l++)
            if (E.out[l].x > 0) cut = std::max(cut, ((uint32_t)E.out[l].y & 0xffff) / (uint32_t)kPairsRows + 1);
        hg[g].nstrips = std::min(cut, hg[g].nstrips);
        rows += block_rows(B, K.g0 + g, hg[g].nstrips);
    }
    check(hipMemcpyAsync((void*)K.A.groups, hg, K.ng * sizeof(BandGroup), hipMemcpyHostToDevice, T.stream),
          "pairs_xdrop groups upload");
    return rows;
}

// the empty alignment: score 0, region zeros, no text
void empty_alignment(ssa_amd_pair_alignment_t& o, char* text) {
    o.score = 0;
    for (auto& r : o.region) r = 0;
    o.cigar_len = 0;
    text[0] = 0;
}

// One pair of the summary call on the host path: the align routine, its text counted in place; true for the
// empty alignment of two non-empty sides.
bool host_summary(int mode, const uint8_t* q, size_t ql, const uint8_t* d, size_t dl, int64_t lo, int64_t hi,
                  int64_t xdrop, std::vector<char>& text, ssa_amd_pair_summary_t& o, bool& dropped) {
    ssa_amd_pair_alignment_t a{};
    if (text.size() < ql + dl + 1) text.resize(ql + dl + 1);
    const bool zero = xdrop_host_align(mode, q, ql, d, dl, lo, hi, xdrop, a, text.data(), dropped);
    o = ssa_amd_pair_summary_t{};
    o.score = a.score;
    o.flags = 1;
    for (int k = 0; k < 4; k++) o.region[k] = a.region[k];
    if (a.cigar_len) summary_count_text(text.data(), q, d, o);
    return zero;
}

}  // namespace

uint64_t xdrop_dropped() { return g_dropped.load(); }

int score_pairs_xdrop(int mode, int64_t xdrop, const int64_t* band_lo, const int64_t* band_hi, const uint8_t* qc,
                      const uint64_t* qoff, const uint8_t* dc, const uint64_t* doff, size_t n, int64_t* scores) {
    const double t0 = now_ms();
    if (check_mode(mode, xdrop, band_lo, band_hi)) return 1;
    std::vector<int64_t> lo, hi;
    if (!ends_args_ok(mode & 15, qc, qoff, dc, doff, n) || (n && !scores)) return 1;
    if (!local_bands_ok(mode, band_lo, band_hi, qoff, doff, n, lo, hi)) return 1;
    ssa_amd_pairs_stats_t S{};
    S.strip_rows = kPairsRows;
    S.device = -1;
    g_dropped = 0;
    if (n == 0) {
        set_pairs_stats(S);
        return 0;
    }
    if (!matrix().ready) fatal("Scoring matrix not initialized");
    EndsRouting T;
    ends_route(T, n);
    S.pairs = n;
    S.device = T.device ? T.dev_id : -1;
    snprintf(S.kernel, sizeof S.kernel, "pairs_xdrop_i32");

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
    std::atomic<uint64_t> drops{0};
    // ---- the host path
    const double th0 = now_ms();
    S.host_pairs = todo.size();
    parallel_ranges(todo.size(), 8, [&](size_t b, size_t e) {
        for (size_t k = b; k < e; k++) {
            const size_t i = todo[k];
            bool dropped = false;
            scores[i] = xdrop_host_score(mode, qc + qoff[i], qoff[i + 1] - qoff[i], dc + doff[i],
                                         doff[i + 1] - doff[i], lo[i], hi[i], xdrop, dropped);
            drops += dropped;
        }
    });
    S.host_ms = now_ms() - th0;

    // ---- the device path
    if (!B.idx.empty()) {
        banded_prepare_device(T.dev_id);
        const double tp0 = now_ms();
        B.order(false);
        S.groups = (uint32_t)B.groups.size();
        S.pack_ms += now_ms() - tp0;
        for (size_t g0 = 0; g0 < B.groups.size();) {
            const double tc0 = now_ms();
            const BandChunk K = banded_pack_chunk(B, g0, false, mode & 15, T);
            S.pack_ms += now_ms() - tc0;
            const EndPass E = end_pass(K, xdrop, T);
            S.kernel_ms += E.ms;
            for (size_t p = K.p0; p < K.p1; p++) scores[B.idx[p]] = E.out[p - K.p0].x;
            drops += count_dropped(K, E);
            // the column blocks of the strips the waves entered
            for (size_t g = 0; g < K.ng; g++)
                S.swept_cells += block_rows(B, K.g0 + g, E.entered[g]) * 4 * kPairsRows * 64;
            S.chunks++;
            S.launches++;
            g0 = K.g1;
        }
    }
    g_dropped = drops.load();
    S.total_ms = now_ms() - t0;
    set_pairs_stats(S);
    return 0;
}

int align_pairs_xdrop(int mode, int64_t xdrop, const int64_t* band_lo, const int64_t* band_hi, const uint8_t* qc,
                      const uint64_t* qoff, const uint8_t* dc, const uint64_t* doff, size_t n,
                      ssa_amd_pair_alignment_t* out, char* cigars, size_t cigar_cap) {
    const double t0 = now_ms();
    if (check_mode(mode, xdrop, band_lo, band_hi)) return 1;
    std::vector<int64_t> lo, hi;
    if (!ends_args_ok(mode & 15, qc, qoff, dc, doff, n) || (n && (!out || !cigars))) return 1;
    if (!local_bands_ok(mode, band_lo, band_hi, qoff, doff, n, lo, hi)) return 1;
    // every pair's CIGAR slot: qlen + dlen + 1 bytes, in input order
    std::vector<uint64_t> coff(n + 1);
    coff[0] = 0;
    for (size_t i = 0; i < n; i++) coff[i + 1] = coff[i] + (qoff[i + 1] - qoff[i]) + (doff[i + 1] - doff[i]) + 1;
    if (cigar_cap < coff[n]) return 1;
    ssa_amd_align_pairs_stats_t S{};
    S.device = -1;
    g_dropped = 0;
    if (n == 0) {
        set_align_pairs_stats(S);
        return 0;
    }
    if (!matrix().ready) fatal("Scoring matrix not initialized");

    EndsRouting T;
    ends_route(T, n);
    S.pairs = n;
    S.device = T.device ? T.dev_id : -1;

    BandBatch B{qc, qoff, dc, doff, lo.data(), hi.data(), {}, {}, {}, {}, {}};
    std::vector<size_t> todo;        // the pairs of the host path
    for (size_t i = 0; i < n; i++) {
        const uint64_t ql = qoff[i + 1] - qoff[i], dl = doff[i + 1] - doff[i];
        S.cells += ql * dl;
        // the local align call's conditions, planned for the whole band: the cut is not known yet
        if (T.device && ql && dl && (int64_t)(ql + dl) <= T.residue_limit && ql < kAlignMaxLen && dl < kAlignMaxLen &&
            pair_dir_rows(ql, dl, lo[i], hi[i]) * kBandDirRowBytes <= kBandPairDirBudget)
            B.idx.push_back((uint32_t)i);
        else
            todo.push_back(i);
    }
    std::atomic<uint64_t> zeros{0}, drops{0};
    auto on_host = [&](size_t i, bool count_drop) {
        bool dropped = false;
        out[i].cigar_off = coff[i];
        if (xdrop_host_align(mode, qc + qoff[i], qoff[i + 1] - qoff[i], dc + doff[i], doff[i + 1] - doff[i], lo[i],
                             hi[i], xdrop, out[i], cigars + coff[i], dropped))
            zeros++;
        if (count_drop) drops += dropped;
    };
    // ---- the host path
    const double th0 = now_ms();
    S.host_pairs = todo.size();
    parallel_ranges(todo.size(), 4, [&](size_t b, size_t e) {
        for (size_t k = b; k < e; k++) on_host(todo[k], true);
    });
    S.host_ms = now_ms() - th0;

    // ---- the device path
    if (!B.idx.empty()) {
        BandedDevice& P = banded_device();
        banded_prepare_device(T.dev_id);
        snprintf(S.kernels, sizeof S.kernels, "pairs_xdrop_end,pairs_local_dir,pairs_local_walk");
        const double tp0 = now_ms();
        B.order(true, kBandDirRowBytes);
        S.groups = (uint32_t)B.groups.size();
        S.pack_ms += now_ms() - tp0;
        for (size_t g0 = 0; g0 < B.groups.size();) {
            const double tc0 = now_ms();
            const BandChunk K = banded_pack_chunk(B, g0, true, mode & 15, T);
            S.pack_ms += now_ms() - tc0;
            // ---- the end cells; then the directions down to the furthest of them, and the walk
            const EndPass E = end_pass(K, xdrop, T);
            S.fwd_ms += E.ms;
            drops += count_dropped(K, E);
            const double tk0 = now_ms();
            S.dir_bytes += cut_groups(B, K, E, T) * kBandDirRowBytes;
            S.pack_ms += now_ms() - tk0;
            LocalArgs A;
            A.b = K.A;
            A.stop = nullptr;
            check(hipEventRecord(P.ev[1], T.stream), "hipEventRecord");
            check(launch_pairs_local(1, mode, A, T.stream), "pairs_local_dir");
            check(hipEventRecord(P.ev[2], T.stream), "hipEventRecord");
            check(launch_pairs_local(2, mode, A, T.stream), "pairs_local_walk");
            check(hipEventRecord(P.ev[3], T.stream), "hipEventRecord");
            check(hipMemcpyAsync(P.out.h, P.out.d, K.nl * (sizeof(int2) + sizeof(uint32_t)), hipMemcpyDeviceToHost,
                                 T.stream),
                  "pairs_xdrop results copy");
            if (K.nruns)
                check(hipMemcpyAsync(P.runs.h, P.runs.d, K.nruns * sizeof(uint32_t), hipMemcpyDeviceToHost, T.stream),
                      "pairs_xdrop runs copy");
            check(hipStreamSynchronize(T.stream), "pairs_xdrop synchronize");
            S.dir_ms += banded_elapsed(1);
            S.walk_ms += banded_elapsed(2);
            S.launches += 3;

            // ---- region and text
            const double tt0 = now_ms();
            const int2* h_out = (const int2*)P.out.h;
            const uint32_t* h_runs = (const uint32_t*)P.runs.h;
            const uint32_t* h_nruns = (const uint32_t*)(h_out + K.nl);
            std::atomic<uint64_t> lost{0};
            parallel_ranges(K.p1 - K.p0, 64, [&](size_t b, size_t e) {
                std::vector<uint32_t> runs;
                for (size_t l = b; l < e; l++) {
                    const AlignLane& L = K.lanes[l];
                    const uint32_t i = B.idx[K.p0 + l];
                    if (h_nruns[l] == kBandWalkLost) {
                        // the walk stood outside what was stored (expected never): the host routine; its drop
                        // row is the one the end pass has counted
                        lost++;
                        on_host(i, false);
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
                    o.cigar_len =
                        ends_finish_alignment(mode & 15, pos & 0xffff, pos >> 16, runs, o.region, cigars + coff[i]);
                }
            });
            S.device_fallbacks += lost.load();
            S.host_pairs += lost.load();
            S.text_ms += now_ms() - tt0;
            S.chunks++;
            g0 = K.g1;
        }
    }
    g_dropped = drops.load();
    S.zero_pairs = zeros.load();
    S.kernel_ms = S.fwd_ms + S.dir_ms + S.walk_ms;
    S.total_ms = now_ms() - t0;
    set_align_pairs_stats(S);
    return 0;
}

int summarize_pairs_xdrop(int mode, int64_t xdrop, const int64_t* band_lo, const int64_t* band_hi, const uint8_t* qc,
                          const uint64_t* qoff, const uint8_t* dc, const uint64_t* doff, size_t n,
                          ssa_amd_pair_summary_t* out) {
    const double t0 = now_ms();
    if (check_mode(mode, xdrop, band_lo, band_hi)) return 1;
    std::vector<int64_t> lo, hi;
    if (!ends_args_ok(mode & 15, qc, qoff, dc, doff, n) || (n && !out)) return 1;
    if (!local_bands_ok(mode, band_lo, band_hi, qoff, doff, n, lo, hi)) return 1;
    ssa_amd_align_pairs_stats_t S{};
    S.device = -1;
    g_dropped = 0;
    if (n == 0) {
        set_align_pairs_stats(S);
        return 0;
    }
    if (!matrix().ready) fatal("Scoring matrix not initialized");
    EndsRouting T;
    ends_route(T, n);
    S.pairs = n;
    S.device = T.device ? T.dev_id : -1;

    BandBatch B{qc, qoff, dc, doff, lo.data(), hi.data(), {}, {}, {}, {}, {}};
    std::vector<size_t> todo;        // the pairs of the host path
    for (size_t i = 0; i < n; i++) {
        const uint64_t ql = qoff[i + 1] - qoff[i], dl = doff[i + 1] - doff[i];
        S.cells += ql * dl;
        // the summary call's conditions; positions travel as 16 + 16 bits
        if (T.device && ql && dl && (int64_t)(ql + dl) <= T.residue_limit && ql < kAlignMaxLen && dl < kAlignMaxLen)
            B.idx.push_back((uint32_t)i);
        else
            todo.push_back(i);
    }
    std::atomic<uint64_t> zeros{0}, drops{0};
    // ---- the host path
    const double th0 = now_ms();
    S.host_pairs = todo.size();
    parallel_ranges(todo.size(), 4, [&](size_t b, size_t e) {
        std::vector<char> text;
        for (size_t k = b; k < e; k++) {
            const size_t i = todo[k];
            bool dropped = false;
            if (host_summary(mode, qc + qoff[i], qoff[i + 1] - qoff[i], dc + doff[i], doff[i + 1] - doff[i], lo[i],
                             hi[i], xdrop, text, out[i], dropped))
                zeros++;
            drops += dropped;
        }
    });
    S.host_ms = now_ms() - th0;

    // ---- the device path
    if (!B.idx.empty()) {
        BandedDevice& P = banded_device();
        banded_prepare_device(T.dev_id);
        snprintf(S.kernels, sizeof S.kernels, "pairs_xdrop_end,pairs_summary_sweep");
        const double tp0 = now_ms();
        B.order(false);
        S.groups = (uint32_t)B.groups.size();
        S.pack_ms += now_ms() - tp0;
        for (size_t g0 = 0; g0 < B.groups.size();) {
            const double tc0 = now_ms();
            const BandChunk K = banded_pack_chunk(B, g0, false, mode & 15, T);
            const uint2* h_sum = nullptr;
            const SummaryArgs A = summary_chunk_args(B, K, T.dev_id, &h_sum);
            S.pack_ms += now_ms() - tc0;
            // ---- the end cells; then the sweep with the words down to the furthest of them
            const EndPass E = end_pass(K, xdrop, T);
            S.fwd_ms += E.ms;
            drops += count_dropped(K, E);
            const double tk0 = now_ms();
            cut_groups(B, K, E, T);
            S.pack_ms += now_ms() - tk0;
            check(hipEventRecord(P.ev[1], T.stream), "hipEventRecord");
            check(launch_pairs_summary(false, true, A, T.stream), "pairs_summary_sweep");
            check(hipEventRecord(P.ev[2], T.stream), "hipEventRecord");
            check(hipMemcpyAsync((void*)h_sum, A.sum, K.nl * sizeof(uint2), hipMemcpyDeviceToHost, T.stream),
                  "pairs_xdrop words copy");
            check(hipStreamSynchronize(T.stream), "pairs_xdrop synchronize");
            S.dir_ms += banded_elapsed(1);
            S.launches += 2;
            // (the end cells are still where the end pass's copy left them)
            uint64_t z = 0;
            for (size_t p = K.p0; p < K.p1; p++)
                z += summary_record(true, E.out[p - K.p0], h_sum[p - K.p0], out[B.idx[p]]);
            zeros += z;
            S.chunks++;
            g0 = K.g1;
        }
    }
    g_dropped = drops.load();
    S.zero_pairs = zeros.load();
    S.kernel_ms = S.fwd_ms + S.dir_ms;
    S.total_ms = now_ms() - t0;
    set_align_pairs_stats(S);
    return 0;
}

}  // namespace ssa
