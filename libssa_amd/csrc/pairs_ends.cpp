// pairs_ends.cpp -- ssa_amd_score_pairs_ends / ssa_amd_align_pairs_ends: the
// ends-free (semi-global) family over a batch of independent pairs (DESIGN.md
// §9.2).  NW's recurrence with a zero boundary where a begin is free and a
// maximum over the last column / last row where an end is free; `ends` is the
// mask of the four SSA_AMD_FREE_* bits.  The batch is ordered and packed as
// ssa_amd_score_pairs packs it (pairs.cpp); a chunk of the score call runs
// ends_kernel<false>, a chunk of the align call ends_kernel<true> (direction
// bits, score, end cell) and ends_walk_kernel, back to back on the stream: the
// walk reads each lane's end cell where the direction kernel left it, so
// there is no host round trip between the two.  What the device does not take
// goes through the int64 routines below, in parallel on the host.  The calls
// share ssa_amd_score_pairs' stream and own their buffers; an open DB, its
// device copy and ssa_amd_get_stats are not touched.
#include <algorithm>
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "pairs_ends.h"
#include "pairs_host.h"

namespace ssa {

// --------------------------------- shared with pairs_banded.cpp (pairs_ends.h)
// The rule among equal candidates: the greatest (d_end, q_end).  The kept
// last-column cell (col_best at row col_row of column dn - 1) has the greatest
// column there is, so the kept last-row cell (row_best at column row_col of row
// qn - 1) wins a tie only as the corner.
EndCell ends_pick_cell(int64_t row_best, size_t row_col, int64_t col_best, size_t col_row, size_t qn, size_t dn) {
    if (row_best > col_best || (row_best == col_best && row_col == dn - 1)) return EndCell{row_best, qn - 1, row_col};
    return EndCell{col_best, col_row, dn - 1};
}

// An empty side: 0 when both are empty or the other side has a free end or begin, else one gap over it.
int64_t ends_empty_score(int ends, size_t qn, size_t dn, int64_t Q, int64_t R) {
    if (qn + dn == 0) return 0;
    const int free_bits = qn == 0 ? (kFreeDBegin | kFreeDEnd) : (kFreeQBegin | kFreeQEnd);
    return (ends & free_bits) ? 0 : Q + (int64_t)(qn + dn) * R;
}

// The region and the text from the end cell and the walk's runs.  The walk
// stands at (i, j) = end cell minus what the runs consumed.  Left through
// column -1 at row i >= 0: a free q begin starts the region at row i + 1,
// else the i + 1 rows above are a leading D run (the boundary's own gap, Q +
// (i + 1) R); the same through row -1 with the d begin and I.  So the CIGAR
// always spans the region and re-scores to the score.
uint32_t ends_finish_alignment(int ends, size_t q_end, size_t d_end, std::vector<uint32_t>& runs, uint64_t region[4],
                               char* text) {
    int64_t qc = 0, dc = 0;
    for (const uint32_t r : runs) {
        if ((r & 3) != kOpI) qc += r >> 2;
        if ((r & 3) != kOpD) dc += r >> 2;
    }
    const int64_t i = (int64_t)q_end - qc, j = (int64_t)d_end - dc;
    uint64_t q_begin = 0, d_begin = 0;
    auto lead = [&](uint32_t op, int64_t n) {
        if (!runs.empty() && (runs.back() & 3) == op) runs.back() += (uint32_t)n << 2;
        else runs.push_back((uint32_t)n << 2 | op);
    };
    if (j < 0 && i >= 0) {
        if (ends & kFreeQBegin) q_begin = (uint64_t)i + 1;
        else lead(kOpD, i + 1);
    } else if (i < 0 && j >= 0) {
        if (ends & kFreeDBegin) d_begin = (uint64_t)j + 1;
        else lead(kOpI, j + 1);
    }
    region[0] = q_begin;
    region[1] = q_end;
    region[2] = d_begin;
    region[3] = d_end;
    return format_runs(runs.data(), (uint32_t)runs.size(), text);
}

// ---------------------------------------------------------------- arguments
// ssa_amd_score_pairs' checks, and the mask's
bool ends_args_ok(int ends, const uint8_t* qc, const uint64_t* qoff, const uint8_t* dc, const uint64_t* doff,
                  size_t n) {
    if (ends < 0 || ends > 15) return false;
    if (n == 0) return true;
    if (!qc || !qoff || !dc || !doff) return false;
    for (size_t i = 0; i < n; i++)
        if (qoff[i + 1] < qoff[i] || doff[i + 1] < doff[i]) return false;
    // every residue is a code < 32 (the matrix is 32 x 32)
    std::atomic<uint32_t> seen{0};
    auto scan = [&](const uint8_t* p, size_t len) {
        parallel_ranges(len, 1 << 20, [&](size_t b, size_t e) {
            uint8_t acc = 0;
            for (size_t i = b; i < e; i++) acc |= p[i];
            seen.fetch_or(acc);
        });
    };
    scan(qc + qoff[0], qoff[n] - qoff[0]);
    scan(dc + doff[0], doff[n] - doff[0]);
    return seen.load() < (uint32_t)kDim;
}

// What the int32 kernels take (pairs.cpp, pairs_align.cpp): an int8 matrix,
// gap penalties <= 0, and per pair at most residue_limit residues.  The bound
// behind the limit, |H|, |E|, |F| <= (qlen + dlen) * (max |M| + |gap_extend|)
// + 2 * |gap_open|, holds unchanged here: a free begin replaces a boundary
// value Q + k R by 0, which is inside it, and an end maximum creates no new
// value.  No symmetric-matrix condition (as for NW: every pass scores M[d][q]).
void ends_route(EndsRouting& T, size_t n) {
    const Config& C = cfg();
    const int64_t* M = matrix().m;
    const int64_t Q = C.gap_open, Ge = C.gap_extend;
    int64_t max_abs = 0;
    bool int8_matrix = true;
    for (int i = 0; i < kDim * kDim; i++) {
        if (M[i] < -128 || M[i] > 127) int8_matrix = false;
        max_abs = std::max<int64_t>(max_abs, std::llabs(M[i]));
    }
    T.device = !C.pairs_host && int8_matrix && Q <= 0 && Ge <= 0 && n <= UINT32_MAX;
    if (T.device) T.device = pairs_use_device(&T.dev_id, &T.stream);
    const int64_t per_residue = max_abs + std::llabs(Ge);
    T.residue_limit = per_residue ? (((int64_t)1 << 29) - 2 * std::llabs(Q)) / per_residue : INT64_MAX;
    if (T.device)
        for (int q = 0; q < kDim; q++)
            for (int d = 0; d < kDim; d++) T.mt[q * 32 + d] = (int8_t)M[(d << 5) + q];
}

namespace {

// ------------------------------------------------------------ the host path
// One pair, both sides non-empty: score and end cell by the definition, in
// int64; he = 2 * qn scratch words.  dir (or nullptr): qn * dn bytes, cell
// (i, j) at dir[j * qn + i], the four kDir* bits -- directions()'s rule
// (align.cpp) under the ends-free boundaries.
EndCell host_ends(int ends, const uint8_t* d, size_t dn, const uint8_t* q, size_t qn, const int64_t* M, int64_t Q,
                  int64_t R, int64_t* he, uint8_t* dir) {
    const bool fqb = ends & kFreeQBegin, fqe = ends & kFreeQEnd, fdb = ends & kFreeDBegin, fde = ends & kFreeDEnd;
    for (size_t i = 0; i < qn; i++) {
        he[2 * i] = fqb ? 0 : Q + (int64_t)(i + 1) * R;      // H(i, -1)
        he[2 * i + 1] = he[2 * i] + Q + R;                    // E(i, 0)
    }
    int64_t row_best = INT64_MIN, col_best = INT64_MIN;
    size_t row_col = 0, col_row = 0;
    for (size_t j = 0; j < dn; j++) {
        const int64_t* row = M + ((size_t)d[j] << 5);
        int64_t f = (fdb ? 0 : Q + (int64_t)(j + 1) * R) + Q + R;          // F(0, j) from H(-1, j)
        int64_t h = (j == 0 || fdb) ? 0 : Q + (int64_t)j * R;              // H(-1, j - 1)
        for (size_t i = 0; i < qn; i++) {
            const int64_t left = he[2 * i];
            const int64_t e = he[2 * i + 1];
            const int64_t diag = h + row[q[i]];
            const int64_t m = std::max(diag, f);
            h = std::max(m, e);
            he[2 * i] = h;
            const int64_t t = h + Q + R, e2 = e + R, f2 = f + R;
            if (dir)
                dir[j * qn + i] = (uint8_t)((e > m ? kDirLeft : 0) | (f > diag ? kDirUp : 0) |
                                            (e2 > t ? kDirExtLeft : 0) | (f2 > t ? kDirExtUp : 0));
            he[2 * i + 1] = std::max(e2, t);
            f = std::max(f2, t);
            h = left;
        }
        // the last row's candidates: every column with a free d end, else the corner; the greatest column wins
        if ((fde || j + 1 == dn) && he[2 * qn - 2] >= row_best) {
            row_best = he[2 * qn - 2];
            row_col = j;
        }
    }
    // the last column's candidates: the greatest row wins
    if (fqe)
        for (size_t i = 0; i < qn; i++)
            if (he[2 * i] >= col_best) {
                col_best = he[2 * i];
                col_row = i;
            }
    return ends_pick_cell(row_best, row_col, col_best, col_row, qn, dn);
}

// The walk (next_op, pairs_ends.h) from the end cell until it leaves the matrix: runs (count << 2 | op)
// in traceback order
void host_walk(const uint8_t* dir, size_t qn, const EndCell& c, std::vector<uint32_t>& runs) {
    runs.clear();
    int64_t i = (int64_t)c.q_end, j = (int64_t)c.d_end;
    uint32_t op = kOpM;
    while (i >= 0 && j >= 0) {
        op = next_op(op, dir[(size_t)j * qn + (size_t)i]);
        if (!runs.empty() && (runs.back() & 3) == op) runs.back() += 4;
        else runs.push_back(1u << 2 | op);
        j -= op != kOpD;
        i -= op != kOpI;
    }
}

// Per-thread scratch of the host path.
struct HostScratch {
    std::vector<int64_t> he;
    std::vector<uint8_t> dir;
    std::vector<uint32_t> runs;
};

int64_t host_score(int ends, const uint8_t* q, size_t ql, const uint8_t* d, size_t dl, HostScratch& W) {
    const int64_t Q = cfg().gap_open, Ge = cfg().gap_extend;
    if (ql == 0 || dl == 0) return ends_empty_score(ends, ql, dl, Q, Ge);
    if (W.he.size() < 2 * ql) W.he.resize(2 * ql);
    return host_ends(ends, d, dl, q, ql, matrix().m, Q, Ge, W.he.data(), nullptr).score;
}

void host_align(int ends, const uint8_t* q, size_t ql, const uint8_t* d, size_t dl, HostScratch& W,
                ssa_amd_pair_alignment_t& o, char* text) {
    const int64_t Q = cfg().gap_open, Ge = cfg().gap_extend;
    o.flags = 1;
    if (ql == 0 || dl == 0) {
        o.score = ends_empty_score(ends, ql, dl, Q, Ge);
        for (auto& r : o.region) r = 0;
        o.cigar_len = 0;
        text[0] = 0;
        return;
    }
    if (W.he.size() < 2 * ql) W.he.resize(2 * ql);
    if (W.dir.size() < ql * dl) W.dir.resize(ql * dl);
    const EndCell c = host_ends(ends, d, dl, q, ql, matrix().m, Q, Ge, W.he.data(), W.dir.data());
    host_walk(W.dir.data(), ql, c, W.runs);
    o.score = c.score;
    o.cigar_len = ends_finish_alignment(ends, c.q_end, c.d_end, W.runs, o.region, text);
}

// ------------------------------------------------------------- device state
constexpr size_t kScoreChunkBudget = (size_t)256 << 20;   // ssa_amd_score_pairs'
// twice ssa_amd_align_pairs': the direction bits dominate, and there are four per cell here.  One launch
// holds 10 000 pairs of 390 x 513 (1.0 GB of bits): a second chunk would be a second full sweep time, since
// that batch is fewer waves than the chip has SIMDs
constexpr size_t kAlignChunkBudget = (size_t)2 << 30;
constexpr size_t kPairDirBudget = (size_t)512 << 20;      // direction bits of one pair alone

struct EndsDevice {
    int device = -1;
    hipEvent_t ev[3] = {};
    bool events = false;
    PairsBuf up, bnd, dir, runs, out;
} g_dev;

void prepare_device(int dev_id) {
    EndsDevice& P = g_dev;
    if (P.device != dev_id) {
        for (PairsBuf* b : {&P.up, &P.bnd, &P.dir, &P.runs, &P.out}) b->release();
        P.device = dev_id;
    }
    if (!P.events) {
        for (auto& e : P.ev) check(hipEventCreate(&e), "hipEventCreate");
        P.events = true;
    }
}

// The device pairs of a call, ordered by shape and cut into groups of 64.
struct Batch {
    const uint8_t* qc;
    const uint64_t* qoff;
    const uint8_t* dc;
    const uint64_t* doff;
    std::vector<uint32_t> idx;          // by input index
    std::vector<AlignGroup> groups;
    std::vector<size_t> gbytes;         // device bytes of each group

    uint32_t qlen(size_t i) const { return (uint32_t)(qoff[i + 1] - qoff[i]); }
    uint32_t dlen(size_t i) const { return (uint32_t)(doff[i + 1] - doff[i]); }
    uint32_t strips(size_t i) const { return (qlen(i) + kPairsRows - 1) / kPairsRows; }

    // a wave sweeps (most strips) x (most columns) of its 64 pairs: order by both, longest first
    // (the last waves of a launch are then the short ones); returns the cells the waves walk
    uint64_t order(bool align) {
        struct Key {
            uint64_t shape;   // strips << 32 | dlen
            uint32_t pair;
        };
        std::vector<Key> keys(idx.size());
        for (size_t p = 0; p < keys.size(); p++) keys[p] = Key{(uint64_t)strips(idx[p]) << 32 | dlen(idx[p]), idx[p]};
        std::sort(keys.begin(), keys.end(),
                  [](const Key& x, const Key& y) { return x.shape != y.shape ? x.shape > y.shape : x.pair < y.pair; });
        for (size_t p = 0; p < keys.size(); p++) idx[p] = keys[p].pair;
        const size_t ngroups = (idx.size() + 63) / 64;
        groups.assign(ngroups, AlignGroup{});
        gbytes.assign(ngroups, 0);
        uint64_t swept = 0;
        for (size_t g = 0; g < ngroups; g++) {
            uint32_t md = 0, ms = 0;
            uint64_t ops = 0;
            for (size_t p = g * 64; p < std::min(idx.size(), g * 64 + 64); p++) {
                md = std::max(md, dlen(idx[p]));
                ms = std::max(ms, strips(idx[p]));
                ops += (uint64_t)qlen(idx[p]) + dlen(idx[p]);
            }
            AlignGroup& G = groups[g];
            G.ncb = (md + 3) / 4;
            G.nstrips = ms;
            swept += (uint64_t)ms * kPairsRows * G.ncb * 4 * 64;
            // residues, bnd, per-lane words; the align call: direction bits and run slots
            gbytes[g] = (size_t)G.ncb * 256 + (size_t)G.nstrips * 512 + (size_t)G.ncb * 4 * 512 +
                        64 * (sizeof(uint2) + sizeof(AlignLane) + sizeof(int2)) + sizeof(AlignGroup);
            if (align) gbytes[g] += (size_t)G.nstrips * G.ncb * 1024 + ops * 4;
        }
        return swept;
    }
};

// One chunk: groups [g0, g1) laid out in the upload block, packed and uploaded.
struct Chunk {
    size_t g0, g1, ng, nl, p0, p1;
    uint64_t drow = 0;                  // the align call: 64-lane uint4 rows of direction bits
    uint64_t nruns = 0;                 //   and run slots
    AlignLane* lanes = nullptr;         //   the host copy of the lanes
    EndsArgs A{};
};

// Cuts the chunk that starts at g0 (within the byte budget, at least one
// group), packs it lane-interleaved into the pinned block and enqueues its
// upload; sizes every device buffer the kernels of the chunk touch.
Chunk pack_chunk(Batch& B, size_t g0, bool align, int ends, const EndsRouting& T) {
    EndsDevice& P = g_dev;
    const Config& C = cfg();
    const size_t ngroups = B.groups.size(), npd = B.idx.size();
    const size_t chunk_groups = C.pairs_chunk > 0 ? std::max<size_t>(1, (size_t)C.pairs_chunk / 64) : SIZE_MAX;
    const size_t budget = align ? kAlignChunkBudget : kScoreChunkBudget;
    Chunk K;
    size_t g1 = g0, bytes = 0;
    uint64_t trow = 0, qrow = 0, brow = 0, drow = 0;
    while (g1 < ngroups && g1 - g0 < chunk_groups) {
        AlignGroup& G = B.groups[g1];
        if (g1 > g0 && bytes + B.gbytes[g1] > budget) break;
        G.t_row = (uint32_t)trow;
        G.q_row = (uint32_t)qrow;
        G.b_row = (uint32_t)brow;
        G.d_row = (uint32_t)drow;
        trow += G.ncb;
        qrow += (uint64_t)G.nstrips * 2;
        brow += (uint64_t)G.ncb * 4;
        if (align) drow += (uint64_t)G.nstrips * G.ncb;
        bytes += B.gbytes[g1];
        g1++;
    }
    K.g0 = g0;
    K.g1 = g1;
    K.ng = g1 - g0;
    K.nl = K.ng * 64;
    K.p0 = g0 * 64;
    K.p1 = std::min(npd, g1 * 64);
    K.drow = drow;
    // the upload block: matrix, groups, lens, lanes (the align call), query and target residues
    const size_t o_groups = pairs_align_up(sizeof T.mt);
    const size_t o_lens = o_groups + pairs_align_up(K.ng * sizeof(AlignGroup));
    const size_t o_lanes = o_lens + pairs_align_up(K.nl * sizeof(uint2));
    const size_t o_q = o_lanes + (align ? pairs_align_up(K.nl * sizeof(AlignLane)) : 0);
    const size_t o_t = o_q + (size_t)qrow * 256;
    const size_t up_bytes = o_t + (size_t)trow * 256;
    P.up.need(up_bytes, true, "pairs_ends residues");
    P.bnd.need((size_t)brow * 512, false, "pairs_ends boundary buffer");
    P.out.need(K.nl * (sizeof(int2) + sizeof(uint32_t)), true, "pairs_ends results");
    if (align) P.dir.need((size_t)drow * 1024, false, "pairs_ends direction bits");

    memcpy(P.up.h, T.mt, sizeof T.mt);
    memcpy(P.up.h + o_groups, &B.groups[g0], K.ng * sizeof(AlignGroup));
    uint2* h_lens = (uint2*)(P.up.h + o_lens);
    parallel_ranges(K.ng, 1, [&](size_t b, size_t e) {
        for (size_t g = g0 + b; g < g0 + e; g++) {
            const AlignGroup& G = B.groups[g];
            uint8_t* tq = P.up.h + o_q + (size_t)G.q_row * 256;
            uint8_t* tt = P.up.h + o_t + (size_t)G.t_row * 256;
            memset(tq, (int)kPairsPad, (size_t)G.nstrips * 2 * 256);
            memset(tt, (int)kPairsPad, (size_t)G.ncb * 256);
            for (size_t l = 0; l < 64; l++) {
                const size_t p = g * 64 + l;
                uint2& L = h_lens[(g - g0) * 64 + l];
                if (p >= npd) {
                    L = make_uint2(0, 0);
                    continue;
                }
                const uint32_t i = B.idx[p];
                L = make_uint2(B.qlen(i), B.dlen(i));
                interleave(tq + l * 4, B.qc + B.qoff[i], B.qlen(i));
                interleave(tt + l * 4, B.dc + B.doff[i], B.dlen(i));
            }
        }
    });
    if (align) {
        // the walk's lanes: a run slot of qlen + dlen each (a walk makes at most that many steps)
        K.lanes = (AlignLane*)(P.up.h + o_lanes);
        memset(K.lanes, 0, K.nl * sizeof(AlignLane));
        uint64_t nruns = 0;
        for (size_t p = K.p0; p < K.p1; p++) {
            AlignLane& L = K.lanes[p - K.p0];
            L.used = 1;
            L.cap = B.qlen(B.idx[p]) + B.dlen(B.idx[p]);
            L.slot = (uint32_t)nruns;
            nruns += L.cap;
        }
        K.nruns = nruns;
        P.runs.need(std::max<size_t>(nruns, 1) * sizeof(uint32_t), true, "pairs_ends runs");
    }
    check(hipMemcpyAsync(P.up.d, P.up.h, up_bytes, hipMemcpyHostToDevice, T.stream), "pairs_ends upload");
    EndsArgs& A = K.A;
    A.mt = (const int8_t*)P.up.d;
    A.groups = (const AlignGroup*)(P.up.d + o_groups);
    A.lens = (const uint2*)(P.up.d + o_lens);
    A.lanes = align ? (const AlignLane*)(P.up.d + o_lanes) : nullptr;
    A.qres = (const uint32_t*)(P.up.d + o_q);
    A.tres = (const uint32_t*)(P.up.d + o_t);
    A.bnd = (int2*)P.bnd.d;
    A.dir = align ? (uint4*)P.dir.d : nullptr;
    A.runs = align ? (uint32_t*)P.runs.d : nullptr;
    A.out = (int2*)P.out.d;
    A.nruns = (uint32_t*)(A.out + K.nl);
    A.gap_open = (int32_t)C.gap_open;
    A.gap_extend = (int32_t)C.gap_extend;
    A.ends = ends;
    A.ngroups = (uint32_t)K.ng;
    return K;
}

double elapsed(int e) {
    float ms = 0;
    check(hipEventElapsedTime(&ms, g_dev.ev[e], g_dev.ev[e + 1]), "hipEventElapsedTime");
    return (double)ms;
}

}  // namespace

int score_pairs_ends(int ends, const uint8_t* qc, const uint64_t* qoff, const uint8_t* dc, const uint64_t* doff,
                     size_t n, int64_t* scores) {
    const double t0 = now_ms();
    if (!ends_args_ok(ends, qc, qoff, dc, doff, n) || (n && !scores)) return 1;
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
    snprintf(S.kernel, sizeof S.kernel, "pairs_ends_i32");

    Batch B{qc, qoff, dc, doff, {}, {}, {}};
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
            scores[i] = host_score(ends, qc + qoff[i], qoff[i + 1] - qoff[i], dc + doff[i], doff[i + 1] - doff[i], W);
        }
    });
    S.host_ms = now_ms() - th0;

    // ---- the device path
    if (!B.idx.empty()) {
        EndsDevice& P = g_dev;
        prepare_device(T.dev_id);
        const double tp0 = now_ms();
        S.swept_cells = B.order(false);
        S.groups = (uint32_t)B.groups.size();
        S.pack_ms += now_ms() - tp0;
        for (size_t g0 = 0; g0 < B.groups.size();) {
            const double tc0 = now_ms();
            const Chunk K = pack_chunk(B, g0, false, ends, T);
            S.pack_ms += now_ms() - tc0;
            check(hipEventRecord(P.ev[0], T.stream), "hipEventRecord");
            check(launch_pairs_ends(0, K.A, T.stream), "pairs_ends_i32");
            check(hipEventRecord(P.ev[1], T.stream), "hipEventRecord");
            check(hipMemcpyAsync(P.out.h, P.out.d, K.nl * sizeof(int2), hipMemcpyDeviceToHost, T.stream),
                  "pairs_ends scores copy");
            check(hipStreamSynchronize(T.stream), "pairs_ends synchronize");
            S.kernel_ms += elapsed(0);
            const int2* h_out = (const int2*)P.out.h;
            for (size_t p = K.p0; p < K.p1; p++) scores[B.idx[p]] = h_out[p - K.p0].x;
            S.chunks++;
            S.launches++;
            g0 = K.g1;
        }
    }
    S.total_ms = now_ms() - t0;
    set_pairs_stats(S);
    return 0;
}

int align_pairs_ends(int ends, const uint8_t* qc, const uint64_t* qoff, const uint8_t* dc, const uint64_t* doff,
                     size_t n, ssa_amd_pair_alignment_t* out, char* cigars, size_t cigar_cap) {
    const double t0 = now_ms();
    if (!ends_args_ok(ends, qc, qoff, dc, doff, n) || (n && (!out || !cigars))) return 1;
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

    Batch B{qc, qoff, dc, doff, {}, {}, {}};
    std::vector<size_t> todo;        // the pairs of the host path
    for (size_t i = 0; i < n; i++) {
        const uint64_t ql = qoff[i + 1] - qoff[i], dl = doff[i + 1] - doff[i];
        S.cells += ql * dl;
        // §9.1's conditions: positions travel as col << 16 | row; the pair's direction bits alone (4 per cell
        // here) are at most 512 MiB
        if (T.device && ql && dl && (int64_t)(ql + dl) <= T.residue_limit && ql < kAlignMaxLen && dl < kAlignMaxLen &&
            ((ql + 7) / 8) * ((dl + 3) / 4) * 1024 <= kPairDirBudget)
            B.idx.push_back((uint32_t)i);
        else
            todo.push_back(i);
    }
    // ---- the host path
    const double th0 = now_ms();
    S.host_pairs = todo.size();
    parallel_ranges(todo.size(), 4, [&](size_t b, size_t e) {
        HostScratch W;
        for (size_t k = b; k < e; k++) {
            const size_t i = todo[k];
            out[i].cigar_off = coff[i];
            host_align(ends, qc + qoff[i], qoff[i + 1] - qoff[i], dc + doff[i], doff[i + 1] - doff[i], W, out[i],
                       cigars + coff[i]);
        }
    });
    S.host_ms = now_ms() - th0;

    // ---- the device path
    if (!B.idx.empty()) {
        EndsDevice& P = g_dev;
        prepare_device(T.dev_id);
        snprintf(S.kernels, sizeof S.kernels, "pairs_ends_dir,pairs_ends_walk");
        const double tp0 = now_ms();
        B.order(true);
        S.groups = (uint32_t)B.groups.size();
        S.pack_ms += now_ms() - tp0;
        for (size_t g0 = 0; g0 < B.groups.size();) {
            const double tc0 = now_ms();
            const Chunk K = pack_chunk(B, g0, true, ends, T);
            S.pack_ms += now_ms() - tc0;
            S.dir_bytes += K.drow * 1024;
            // ---- directions (with the score and the end cell), then the walk from that end cell
            check(hipEventRecord(P.ev[0], T.stream), "hipEventRecord");
            check(launch_pairs_ends(1, K.A, T.stream), "pairs_ends_dir");
            check(hipEventRecord(P.ev[1], T.stream), "hipEventRecord");
            check(launch_pairs_ends(2, K.A, T.stream), "pairs_ends_walk");
            check(hipEventRecord(P.ev[2], T.stream), "hipEventRecord");
            check(hipMemcpyAsync(P.out.h, P.out.d, K.nl * (sizeof(int2) + sizeof(uint32_t)), hipMemcpyDeviceToHost,
                                 T.stream),
                  "pairs_ends results copy");
            if (K.nruns)
                check(hipMemcpyAsync(P.runs.h, P.runs.d, K.nruns * sizeof(uint32_t), hipMemcpyDeviceToHost, T.stream),
                      "pairs_ends runs copy");
            check(hipStreamSynchronize(T.stream), "pairs_ends synchronize");
            S.dir_ms += elapsed(0);
            S.walk_ms += elapsed(1);
            S.launches += 2;

            // ---- region and text
            const double tt0 = now_ms();
            const int2* h_out = (const int2*)P.out.h;
            const uint32_t* h_runs = (const uint32_t*)P.runs.h;
            const uint32_t* h_nruns = (const uint32_t*)(h_out + K.nl);
            parallel_ranges(K.p1 - K.p0, 64, [&](size_t b, size_t e) {
                std::vector<uint32_t> runs;
                for (size_t l = b; l < e; l++) {
                    const AlignLane& L = K.lanes[l];
                    const uint32_t i = B.idx[K.p0 + l];
                    ssa_amd_pair_alignment_t& o = out[i];
                    o.cigar_off = coff[i];
                    o.flags = 0;
                    o.score = h_out[l].x;
                    const uint32_t pos = (uint32_t)h_out[l].y;
                    const uint32_t nr = std::min(h_nruns[l], L.cap);
                    runs.assign(h_runs + L.slot, h_runs + L.slot + nr);
                    o.cigar_len =
                        ends_finish_alignment(ends, pos & 0xffff, pos >> 16, runs, o.region, cigars + coff[i]);
                }
            });
            S.text_ms += now_ms() - tt0;
            S.chunks++;
            g0 = K.g1;
        }
    }
    S.kernel_ms = S.dir_ms + S.walk_ms;
    S.total_ms = now_ms() - t0;
    set_align_pairs_stats(S);
    return 0;
}

}  // namespace ssa
