// pairs_summary.cpp -- ssa_amd_summarize_pairs_local: score, region and the
// column counts of ssa_amd_align_pairs_local's alignment without its
// traceback.  Packing, ordering and chunking are the score
// calls' (pairs_banded_host.h: BandBatch::order(false), banded_pack_chunk
// without the align buffers, 256 MiB a chunk); a NULL band is the full range
// of every pair, under every mode.  A chunk runs two launches back to back:
// the existing score pass, which leaves (score, end cell) per lane in out, and
// summary_kernel (pairs_summary.hip), which repeats the sweep with the words
// and captures them at that cell; one synchronisation per chunk.  What the
// device does not take goes through the existing host align routine, whose
// text is counted in place.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "pairs_banded_host.h"
#include "pairs_summary.h"

namespace ssa {

namespace {

// columns, matched and identical of a CIGAR text walked from (region[0], region[2])
void count_text(const char* text, const uint8_t* q, const uint8_t* d, ssa_amd_pair_summary_t& o) {
    uint64_t i = o.region[0], j = o.region[2];
    for (const char* p = text; *p;) {
        uint32_t cnt = 0;
        for (; *p >= '0' && *p <= '9'; p++) cnt = cnt * 10 + (uint32_t)(*p - '0');
        if (!cnt) cnt = 1;          // a count of 1 is omitted
        const char op = *p++;
        o.columns += cnt;
        if (op == 'M') {
            o.matched += cnt;
            for (uint32_t k = 0; k < cnt; k++) o.identical += q[i + k] == d[j + k];
            i += cnt;
            j += cnt;
        } else if (op == 'I') {
            j += cnt;
        } else {
            i += cnt;
        }
    }
}

// One pair on the host path: the align routine of the canonical mode, its text counted in place; true for
// the empty alignment of two non-empty sides under a local bit.
bool host_summary(int mode, const uint8_t* q, size_t ql, const uint8_t* d, size_t dl, int64_t lo, int64_t hi,
                  std::vector<char>& text, ssa_amd_pair_summary_t& o) {
    ssa_amd_pair_alignment_t a{};
    if (text.size() < ql + dl + 1) text.resize(ql + dl + 1);
    bool zero = false;
    if (mode < 16)
        banded_host_align(mode, q, ql, d, dl, lo, hi, a, text.data());
    else
        zero = local_host_align(mode, q, ql, d, dl, lo, hi, a, text.data());
    o = ssa_amd_pair_summary_t{};
    o.score = a.score;
    o.flags = 1;
    for (int k = 0; k < 4; k++) o.region[k] = a.region[k];
    if (a.cigar_len) count_text(text.data(), q, d, o);
    return zero;
}

// One device pair's record from its end cell and its words; true for the empty alignment under a local bit.
bool record_of(bool local, const int2 e, const uint2 w, ssa_amd_pair_summary_t& o) {
    o = ssa_amd_pair_summary_t{};
    if (local && e.x <= 0) return true;
    const uint32_t pos = (uint32_t)e.y;
    o.score = e.x;
    o.region[0] = w.y >> 16;
    o.region[1] = pos & 0xffff;
    o.region[2] = w.y & 0xffff;
    o.region[3] = pos >> 16;
    o.matched = w.x & 0xffff;
    o.identical = w.x >> 16;
    // every M column spans one row and one column, every gap column one of the two
    o.columns = (uint32_t)((int64_t)(o.region[1] - o.region[0] + 1) + (int64_t)(o.region[3] - o.region[2] + 1) -
                           (int64_t)o.matched);
    return false;
}

// the row buffer of the words and the lanes' summary words, kept between calls beside banded_device()'s
struct SummaryDevice {
    int device = -1;
    PairsBuf rows, sum;
} g_dev;

SummaryArgs summary_args(const std::vector<BandGroup>& groups, const BandChunk& K, int dev_id) {
    SummaryDevice& P = g_dev;
    if (P.device != dev_id) {
        P.rows.release();
        P.sum.release();
        P.device = dev_id;
    }
    // as many 64-lane rows as the chunk's bnd has: four per column block of every group
    uint64_t brow = 0;
    for (size_t g = K.g0; g < K.g1; g++) brow += (uint64_t)groups[g].ncb * 4;
    P.rows.need(std::max<size_t>((size_t)brow, 1) * 64 * sizeof(uint4), false, "pairs_summary row buffer");
    P.sum.need(K.nl * sizeof(uint2), true, "pairs_summary results");
    SummaryArgs A;
    A.b = K.A;
    A.rows = (uint4*)P.rows.d;
    A.sum = (uint2*)P.sum.d;
    return A;
}

}  // namespace

// ---- shared with pairs_xdrop.cpp (pairs_banded_host.h)
SummaryArgs summary_chunk_args(const std::vector<BandGroup>& groups, const BandChunk& K, int dev_id,
                               const uint2** h_sum) {
    const SummaryArgs A = summary_args(groups, K, dev_id);
    *h_sum = (const uint2*)g_dev.sum.h;
    return A;
}

SummaryArgs summary_chunk_args(const BandBatch& B, const BandChunk& K, int dev_id, const uint2** h_sum) {
    return summary_chunk_args(B.groups, K, dev_id, h_sum);
}

bool summary_record(bool local, int2 end, uint2 words, ssa_amd_pair_summary_t& o) {
    return record_of(local, end, words, o);
}

void summary_count_text(const char* text, const uint8_t* q, const uint8_t* d, ssa_amd_pair_summary_t& o) {
    count_text(text, q, d, o);
}

int summarize_pairs_local(int mode, const int64_t* band_lo, const int64_t* band_hi, const uint8_t* qc,
                          const uint64_t* qoff, const uint8_t* dc, const uint64_t* doff, size_t n,
                          ssa_amd_pair_summary_t* out) {
    const double t0 = now_ms();
    if (mode < 0 || mode > 63 || !band_lo != !band_hi) return 1;
    mode = local_canonical(mode);
    const bool local = mode >= 16;
    std::vector<int64_t> lo, hi;
    if (!ends_args_ok(mode & 15, qc, qoff, dc, doff, n) || (n && !out)) return 1;
    if (!local_bands_ok(mode, band_lo, band_hi, qoff, doff, n, lo, hi)) return 1;
    ssa_amd_align_pairs_stats_t S{};
    S.device = -1;
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
        // the score call's conditions; positions travel as 16 + 16 bits
        if (T.device && ql && dl && (int64_t)(ql + dl) <= T.residue_limit && ql < kAlignMaxLen && dl < kAlignMaxLen)
            B.idx.push_back((uint32_t)i);
        else
            todo.push_back(i);
    }
    std::atomic<uint64_t> zeros{0};
    // ---- the host path
    const double th0 = now_ms();
    S.host_pairs = todo.size();
    parallel_ranges(todo.size(), 4, [&](size_t b, size_t e) {
        std::vector<char> text;
        for (size_t k = b; k < e; k++) {
            const size_t i = todo[k];
            if (host_summary(mode, qc + qoff[i], qoff[i + 1] - qoff[i], dc + doff[i], doff[i + 1] - doff[i], lo[i],
                             hi[i], text, out[i]))
                zeros++;
        }
    });
    S.host_ms = now_ms() - th0;

    // ---- the device path
    if (!B.idx.empty()) {
        BandedDevice& P = banded_device();
        banded_prepare_device(T.dev_id);
        snprintf(S.kernels, sizeof S.kernels, "pairs_summary_end,pairs_summary_sweep");
        const double tp0 = now_ms();
        B.order(false);
        S.groups = (uint32_t)B.groups.size();
        S.pack_ms += now_ms() - tp0;
        for (size_t g0 = 0; g0 < B.groups.size();) {
            const double tc0 = now_ms();
            const BandChunk K = banded_pack_chunk(B, g0, false, mode & 15, T);
            const SummaryArgs A = summary_args(B.groups, K, T.dev_id);
            S.pack_ms += now_ms() - tc0;
            // ---- the end cells, then the sweep with the words, captured at out's end cells
            check(hipEventRecord(P.ev[0], T.stream), "hipEventRecord");
            if (local) {
                LocalArgs LA;
                LA.b = K.A;
                LA.stop = nullptr;
                check(launch_pairs_local(0, mode, LA, T.stream), "pairs_summary_end");
            } else {
                check(launch_pairs_banded(0, K.A, T.stream), "pairs_summary_end");
            }
            check(hipEventRecord(P.ev[1], T.stream), "hipEventRecord");
            check(launch_pairs_summary(mode & kLocalBegin, local, A, T.stream), "pairs_summary_sweep");
            check(hipEventRecord(P.ev[2], T.stream), "hipEventRecord");
            check(hipMemcpyAsync(P.out.h, P.out.d, K.nl * sizeof(int2), hipMemcpyDeviceToHost, T.stream),
                  "pairs_summary end cells copy");
            check(hipMemcpyAsync(g_dev.sum.h, g_dev.sum.d, K.nl * sizeof(uint2), hipMemcpyDeviceToHost, T.stream),
                  "pairs_summary words copy");
            check(hipStreamSynchronize(T.stream), "pairs_summary synchronize");
            S.fwd_ms += banded_elapsed(0);
            S.dir_ms += banded_elapsed(1);
            S.launches += 2;

            const int2* h_out = (const int2*)P.out.h;
            const uint2* h_sum = (const uint2*)g_dev.sum.h;
            uint64_t z = 0;
            for (size_t p = K.p0; p < K.p1; p++)
                z += record_of(local, h_out[p - K.p0], h_sum[p - K.p0], out[B.idx[p]]);
            zeros += z;
            S.chunks++;
            g0 = K.g1;
        }
    }
    S.zero_pairs = zeros.load();
    S.kernel_ms = S.fwd_ms + S.dir_ms;
    S.total_ms = now_ms() - t0;
    set_align_pairs_stats(S);
    return 0;
}

}  // namespace ssa
