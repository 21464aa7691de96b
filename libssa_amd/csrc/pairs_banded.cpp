// pairs_banded.cpp -- ssa_amd_score_pairs_banded / ssa_amd_align_pairs_banded:
// the ends-free family (pairs_ends.cpp) restricted, pair by
// pair, to a band of diagonals k = column - row, lo <= k <= hi (DESIGN.md
// §9.3).  A cell outside the band does not exist: its H, E and F are minus
// infinity; everything else -- boundaries, candidates, tie rule, walk -- is the
// ends calls', over existing cells.  The batch is packed as pairs_ends.cpp
// packs it, ordered so that the lanes of a wave have similar bands, and every
// (group, strip) gets the range of column blocks that holds its lanes'
// in-band columns: the wave sweeps only that range, and the align call keeps
// direction bits only for it.  A chunk of the score call runs
// banded_kernel<false>, a chunk of the align call banded_kernel<true> and
// banded_walk_kernel back to back.  What the device does not take goes
// through the int64 routine below, which keeps H, F and its direction bytes
// for the band only (rows x band width), in parallel on the host.  The band's
// rule, the ordered batch, the chunk packer and the device buffers are declared
// in pairs_banded_host.h: the local pair calls (pairs_local.cpp) use them too.
#include <algorithm>
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "pairs_banded_host.h"

namespace ssa {

// ------------------------------------------------------------------ the band
// Diagonals of a pair's cells, boundaries included, lie in [-qlen, dlen]; values
// beyond are equivalent to the clamped ones (one step further out keeps an
// empty or outlying band what it is).
int64_t clamp_band(int64_t k, uint64_t ql, uint64_t dl) {
    return std::max<int64_t>(-(int64_t)ql - 1, std::min<int64_t>((int64_t)dl + 1, k));
}

// A band admits an alignment iff it is an interval that meets the diagonals an
// alignment may start on and those it may end on (include/libssa_amd.h).
bool band_valid(int ends, int64_t m, int64_t n, int64_t lo, int64_t hi) {
    if (lo > hi) return false;
    const int64_t s_lo = (ends & kFreeQBegin) ? -m : 0, s_hi = (ends & kFreeDBegin) ? n : 0;
    const int64_t e_lo = (ends & kFreeDEnd) ? -(m - 1) : n - m, e_hi = (ends & kFreeQEnd) ? n - 1 : n - m;
    return lo <= s_hi && hi >= s_lo && lo <= e_hi && hi >= e_lo;
}

namespace {

// ------------------------------------------------------------ the host path
constexpr int64_t kNeg = INT64_MIN / 4;     // minus infinity: room for every sum that starts from it

// Per-thread scratch of the host path.
struct HostScratch {
    std::vector<int64_t> h, f;      // band width + 1 words each
    std::vector<uint8_t> dir;       // rows x band width
    std::vector<uint32_t> runs;
};

// One pair, both sides non-empty, a valid clamped band: score and end cell by
// the definition, in int64, row by row.  Row i keeps its cells by k = j - i -
// lo in [0, W): h[k] is H(i, j) once written and H(i - 1, j - 1) -- the
// diagonal -- before; f[k + 1] the F entering (i, j) from (i - 1, j); index W
// is the cell above the band's upper edge, minus infinity.  Column -1 takes
// its place in the row where it is in the band.  dir (or nullptr): qn * W
// bytes, cell (i, j) at dir[i * W + k], host_ends' four bits.
EndCell host_banded(int ends, const uint8_t* q, size_t qn, const uint8_t* d, size_t dn, int64_t lo, int64_t hi,
                    const int64_t* M, int64_t Q, int64_t R, int64_t* h, int64_t* f, uint8_t* dir) {
    const bool fqb = ends & kFreeQBegin, fqe = ends & kFreeQEnd, fdb = ends & kFreeDBegin, fde = ends & kFreeDEnd;
    const int64_t m = (int64_t)qn, n = (int64_t)dn, W = hi - lo + 1, goe = Q + R;
    auto in_band = [&](int64_t k) { return k >= lo && k <= hi; };
    // a boundary whose begin is not free is a gap from (-1, -1): it needs diagonal 0
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
    int64_t row_best = INT64_MIN, col_best = INT64_MIN;
    size_t row_col = 0, col_row = 0;
    for (int64_t i = 0; i < m; i++) {
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
            const int64_t hv = std::max(mx, e);
            h[k] = hv;
            const int64_t t = hv + goe, e2 = e + R, f2 = fv + R;
            if (drow)
                drow[k] = (uint8_t)((e > mx ? kDirLeft : 0) | (fv > diag ? kDirUp : 0) | (e2 > t ? kDirExtLeft : 0) |
                                    (f2 > t ? kDirExtUp : 0));
            e = std::max(e2, t);
            f[k] = std::max(f2, t);
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
    }
    return ends_pick_cell(row_best, row_col, col_best, col_row, qn, dn);
}

// The walk (next_op) from the end cell until it leaves the matrix.  Every cell
// it visits has a finite H and so lies in the band; false if it ever does not.
bool host_walk(const uint8_t* dir, int64_t lo, int64_t W, const EndCell& c, std::vector<uint32_t>& runs) {
    runs.clear();
    int64_t i = (int64_t)c.q_end, j = (int64_t)c.d_end;
    uint32_t op = kOpM;
    while (i >= 0 && j >= 0) {
        const int64_t k = j - i - lo;
        if (k < 0 || k >= W) return false;
        op = next_op(op, dir[(size_t)i * (size_t)W + (size_t)k]);
        if (!runs.empty() && (runs.back() & 3) == op) runs.back() += 4;
        else runs.push_back(1u << 2 | op);
        j -= op != kOpD;
        i -= op != kOpI;
    }
    return true;
}

int64_t host_score(int ends, const uint8_t* q, size_t ql, const uint8_t* d, size_t dl, int64_t lo, int64_t hi,
                   HostScratch& S) {
    const int64_t Q = cfg().gap_open, Ge = cfg().gap_extend;
    if (ql == 0 || dl == 0) return ends_empty_score(ends, ql, dl, Q, Ge);
    const size_t W = (size_t)(hi - lo + 1);
    if (S.h.size() < W + 1) S.h.resize(W + 1), S.f.resize(W + 1);
    return host_banded(ends, q, ql, d, dl, lo, hi, matrix().m, Q, Ge, S.h.data(), S.f.data(), nullptr).score;
}

void host_align(int ends, const uint8_t* q, size_t ql, const uint8_t* d, size_t dl, int64_t lo, int64_t hi,
                HostScratch& S, ssa_amd_pair_alignment_t& o, char* text) {
    const int64_t Q = cfg().gap_open, Ge = cfg().gap_extend;
    o.flags = 1;
    if (ql == 0 || dl == 0) {
        o.score = ends_empty_score(ends, ql, dl, Q, Ge);
        for (auto& r : o.region) r = 0;
        o.cigar_len = 0;
        text[0] = 0;
        return;
    }
    const size_t W = (size_t)(hi - lo + 1);
    if (S.h.size() < W + 1) S.h.resize(W + 1), S.f.resize(W + 1);
    if (S.dir.size() < ql * W) S.dir.resize(ql * W);
    const EndCell c = host_banded(ends, q, ql, d, dl, lo, hi, matrix().m, Q, Ge, S.h.data(), S.f.data(), S.dir.data());
    if (!host_walk(S.dir.data(), lo, (int64_t)W, c, S.runs)) fatal("pairs_banded: the walk left the band");
    o.score = c.score;
    o.cigar_len = ends_finish_alignment(ends, c.q_end, c.d_end, S.runs, o.region, text);
}

// ---------------------------------------------------------------- arguments
// The ends calls' checks and the bands': clamps every band into lo / hi;
// false for a pair of two non-empty sides whose band admits no alignment.
bool bands_ok(int ends, const int64_t* band_lo, const int64_t* band_hi, const uint64_t* qoff, const uint64_t* doff,
              size_t n, std::vector<int64_t>& lo, std::vector<int64_t>& hi) {
    if (n == 0) return true;
    if (!band_lo || !band_hi) return false;
    lo.resize(n);
    hi.resize(n);
    for (size_t i = 0; i < n; i++) {
        const uint64_t ql = qoff[i + 1] - qoff[i], dl = doff[i + 1] - doff[i];
        lo[i] = clamp_band(band_lo[i], ql, dl);
        hi[i] = clamp_band(band_hi[i], ql, dl);
        if (ql && dl && !band_valid(ends, (int64_t)ql, (int64_t)dl, lo[i], hi[i])) return false;
    }
    return true;
}

// ------------------------------------------------------------- device state
BandedDevice g_dev;

}  // namespace

BandedDevice& banded_device() { return g_dev; }

void banded_prepare_device(int dev_id) {
    BandedDevice& P = g_dev;
    if (P.device != dev_id) {
        for (PairsBuf* b : {&P.up, &P.bnd, &P.dir, &P.runs, &P.out, &P.stop}) b->release();
        P.device = dev_id;
    }
    if (!P.events) {
        for (auto& e : P.ev) check(hipEventCreate(&e), "hipEventCreate");
        P.events = true;
    }
}

// 64-lane uint4 rows of direction bits a pair needs when it is alone in its group (an upper bound: its
// in-band columns of a strip span at most 8 + hi - lo columns, and never more than the pair has)
uint64_t pair_dir_rows(uint64_t ql, uint64_t dl, int64_t lo, int64_t hi) {
    const uint64_t blocks = std::min<uint64_t>((dl + 3) / 4, (uint64_t)(hi - lo + 8) / 4 + 2);
    return (ql + 7) / 8 * blocks;
}

namespace {

// A wave sweeps, strip by strip, the union of its lanes' in-band columns: order by strip count
// (longest first), then by the band's position, so that the union is little wider than one lane's.
// Batch: the length source (BandBatch: offsets; BandDescBatch: descriptors), one instantiation each.
template <class Batch>
uint64_t order_batch(Batch& B, bool align, size_t row_bytes) {
    auto& idx = B.idx;
    auto& groups = B.groups;
    auto& strips = B.strips;
    auto& drows = B.drows;
    auto& gbytes = B.gbytes;
    const int64_t* lo = B.lo;
    const int64_t* hi = B.hi;
    auto nstrips = [&](size_t i) { return B.nstrips(i); };
    auto qlen = [&](size_t i) { return B.qlen(i); };
    auto dlen = [&](size_t i) { return B.dlen(i); };
    struct Key {
        uint32_t strips;
        int64_t lo, hi;
        uint32_t pair;
    };
    std::vector<Key> keys(idx.size());
    for (size_t p = 0; p < keys.size(); p++) keys[p] = Key{nstrips(idx[p]), lo[idx[p]], hi[idx[p]], idx[p]};
    std::sort(keys.begin(), keys.end(), [](const Key& x, const Key& y) {
        if (x.strips != y.strips) return x.strips > y.strips;
        if (x.lo != y.lo) return x.lo < y.lo;
        if (x.hi != y.hi) return x.hi < y.hi;
        return x.pair < y.pair;
    });
    for (size_t p = 0; p < keys.size(); p++) idx[p] = keys[p].pair;
    const size_t ngroups = (idx.size() + 63) / 64;
    groups.assign(ngroups, BandGroup{});
    drows.assign(ngroups, 0);
    gbytes.assign(ngroups, 0);
    strips.clear();
    uint64_t swept = 0;
    for (size_t g = 0; g < ngroups; g++) {
        const size_t p0 = g * 64, p1 = std::min(idx.size(), g * 64 + 64);
        uint32_t md = 0, ms = 0;
        uint64_t ops = 0;
        for (size_t p = p0; p < p1; p++) {
            md = std::max(md, dlen(idx[p]));
            ms = std::max(ms, nstrips(idx[p]));
            ops += (uint64_t)qlen(idx[p]) + dlen(idx[p]);
        }
        BandGroup& G = groups[g];
        G.ncb = (md + 3) / 4;
        G.nstrips = ms;
        G.s_row = (uint32_t)strips.size();
        // the strips' ranges: the union over the lanes that have the strip of [8 s + lo, 8 s + 7 + hi] inside
        // the lane's own columns (signed arithmetic: a range may be empty on either side)
        uint64_t rows = 0;
        for (uint32_t s = 0; s < ms; s++) {
            int64_t a = INT64_MAX, b = -1;
            for (size_t p = p0; p < p1; p++) {
                const uint32_t i = idx[p];
                if (nstrips(i) <= s) continue;
                const int64_t ca = std::max<int64_t>(0, (int64_t)s * kPairsRows + lo[i]);
                const int64_t cb = std::min<int64_t>((int64_t)dlen(i) - 1, (int64_t)s * kPairsRows + 7 + hi[i]);
                if (ca > cb) continue;
                a = std::min(a, ca);
                b = std::max(b, cb);
            }
            BandStrip S{};
            if (a <= b) {
                S.cb0 = (uint32_t)(a / 4);
                S.ncb = (uint32_t)(b / 4) + 1 - S.cb0;
            }
            S.d_off = (uint32_t)rows;
            rows += S.ncb;
            strips.push_back(S);
        }
        drows[g] = rows;
        swept += rows * 4 * kPairsRows * 64;
        // residues, bnd, the strip table, per-lane words; the align call: direction bits and run slots
        gbytes[g] = (size_t)G.ncb * 256 + (size_t)G.nstrips * 512 + (size_t)G.ncb * 4 * 512 +
                    (size_t)ms * sizeof(BandStrip) +
                    64 * (sizeof(uint2) + sizeof(int2) + sizeof(AlignLane) + sizeof(int2)) + sizeof(BandGroup);
        if (align) gbytes[g] += (size_t)rows * row_bytes + ops * 4;
    }
    return swept;
}

// Cuts the chunk that starts at g0 (within the byte budget, at least one
// group), packs it lane-interleaved into the pinned block and enqueues its
// upload; sizes every device buffer the kernels of the chunk touch.
// kResidues false (BandDescBatch): the same block without the residue rows and
// the lens -- a device-side packer writes those into a buffer of the caller's
// -- and with the batch's descriptor of every lane behind the bands.
template <bool kResidues, class Batch>
BandChunk pack_chunk(Batch& B, size_t g0, bool align, int ends, const EndsRouting& T) {
    BandedDevice& P = g_dev;
    const Config& C = cfg();
    const size_t ngroups = B.groups.size(), npd = B.idx.size();
    const size_t chunk_groups = C.pairs_chunk > 0 ? std::max<size_t>(1, (size_t)C.pairs_chunk / 64) : SIZE_MAX;
    const size_t budget = align ? kBandAlignChunkBudget : kBandScoreChunkBudget;
    BandChunk K;
    size_t g1 = g0, bytes = 0;
    uint64_t trow = 0, qrow = 0, brow = 0, drow = 0, srow = 0;
    const uint32_t s_first = B.groups[g0].s_row;
    std::vector<BandGroup> cg;          // the chunk's groups, rows relative to the chunk
    while (g1 < ngroups && g1 - g0 < chunk_groups) {
        if (g1 > g0 && bytes + B.gbytes[g1] > budget) break;
        // (a chunk's direction rows are indexed with 32 bits)
        if (g1 > g0 && align && drow + B.drows[g1] > UINT32_MAX) break;
        BandGroup G = B.groups[g1];
        G.t_row = (uint32_t)trow;
        G.q_row = (uint32_t)qrow;
        G.b_row = (uint32_t)brow;
        G.d_row = (uint32_t)drow;
        G.s_row = B.groups[g1].s_row - s_first;
        trow += G.ncb;
        qrow += (uint64_t)G.nstrips * 2;
        brow += (uint64_t)G.ncb * 4;
        srow += G.nstrips;
        if (align) drow += B.drows[g1];
        bytes += B.gbytes[g1];
        cg.push_back(G);
        g1++;
    }
    K.g0 = g0;
    K.g1 = g1;
    K.ng = g1 - g0;
    K.nl = K.ng * 64;
    K.p0 = g0 * 64;
    K.p1 = std::min(npd, g1 * 64);
    K.drow = drow;
    K.qrow = qrow;
    K.trow = trow;
    // the upload block: matrix, groups, strips, lens, bands, lanes (the align call), query and target residues
    // (without residues: matrix, groups, strips, bands, descriptors)
    const size_t o_groups = pairs_align_up(sizeof T.mt);
    const size_t o_strips = o_groups + pairs_align_up(K.ng * sizeof(BandGroup));
    const size_t o_lens = o_strips + pairs_align_up((size_t)srow * sizeof(BandStrip));
    const size_t o_band = o_lens + (kResidues ? pairs_align_up(K.nl * sizeof(uint2)) : 0);
    const size_t o_lanes = o_band + pairs_align_up(K.nl * sizeof(int2));
    const size_t o_q = o_lanes + (align ? pairs_align_up(K.nl * sizeof(AlignLane)) : 0);
    const size_t o_t = o_q + (kResidues ? (size_t)qrow * 256 : pairs_align_up(K.nl * sizeof(HitDesc)));
    const size_t up_bytes = kResidues ? o_t + (size_t)trow * 256 : o_t;
    K.up_bytes = up_bytes;
    P.up.need(up_bytes, true, "pairs_banded residues");
    P.bnd.need((size_t)brow * 512, false, "pairs_banded boundary buffer");
    P.out.need(K.nl * (sizeof(int2) + sizeof(uint32_t)), true, "pairs_banded results");
    if (align) P.dir.need(std::max<size_t>((size_t)drow, 1) * 1024, false, "pairs_banded direction bits");

    memcpy(P.up.h, T.mt, sizeof T.mt);
    memcpy(P.up.h + o_groups, cg.data(), K.ng * sizeof(BandGroup));
    memcpy(P.up.h + o_strips, B.strips.data() + s_first, (size_t)srow * sizeof(BandStrip));
    int2* h_band = (int2*)(P.up.h + o_band);
    if constexpr (kResidues) {
        uint2* h_lens = (uint2*)(P.up.h + o_lens);
        parallel_ranges(K.ng, 1, [&](size_t b, size_t e) {
            for (size_t g = g0 + b; g < g0 + e; g++) {
                const BandGroup& G = cg[g - g0];
                uint8_t* tq = P.up.h + o_q + (size_t)G.q_row * 256;
                uint8_t* tt = P.up.h + o_t + (size_t)G.t_row * 256;
                memset(tq, (int)kPairsPad, (size_t)G.nstrips * 2 * 256);
                memset(tt, (int)kPairsPad, (size_t)G.ncb * 256);
                for (size_t l = 0; l < 64; l++) {
                    const size_t p = g * 64 + l;
                    uint2& L = h_lens[(g - g0) * 64 + l];
                    int2& W = h_band[(g - g0) * 64 + l];
                    if (p >= npd) {
                        L = make_uint2(0, 0);
                        W = make_int2(0, 0);
                        continue;
                    }
                    const uint32_t i = B.idx[p];
                    L = make_uint2(B.qlen(i), B.dlen(i));
                    W = make_int2((int)B.lo[i], (int)B.hi[i]);
                    interleave(tq + l * 4, B.qc + B.qoff[i], B.qlen(i));
                    interleave(tt + l * 4, B.dc + B.doff[i], B.dlen(i));
                }
            }
        });
    } else {
        // (an unused lane's descriptor is all zero)
        HitDesc* h_desc = (HitDesc*)(P.up.h + o_q);
        for (size_t l = 0; l < K.nl; l++) {
            const size_t p = K.p0 + l;
            h_band[l] = p < npd ? make_int2((int)B.lo[B.idx[p]], (int)B.hi[B.idx[p]]) : make_int2(0, 0);
            h_desc[l] = p < npd ? B.desc[B.idx[p]] : HitDesc{0, 0, 0, 0};
        }
        K.desc = (const HitDesc*)(P.up.d + o_q);
    }
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
        P.runs.need(std::max<size_t>(nruns, 1) * sizeof(uint32_t), true, "pairs_banded runs");
    }
    check(hipMemcpyAsync(P.up.d, P.up.h, up_bytes, hipMemcpyHostToDevice, T.stream), "pairs_banded upload");
    BandedArgs& A = K.A;
    A.mt = (const int8_t*)P.up.d;
    A.groups = (const BandGroup*)(P.up.d + o_groups);
    A.strips = (const BandStrip*)(P.up.d + o_strips);
    A.lens = kResidues ? (const uint2*)(P.up.d + o_lens) : nullptr;
    A.band = (const int2*)(P.up.d + o_band);
    A.lanes = align ? (const AlignLane*)(P.up.d + o_lanes) : nullptr;
    A.qres = kResidues ? (const uint32_t*)(P.up.d + o_q) : nullptr;
    A.tres = kResidues ? (const uint32_t*)(P.up.d + o_t) : nullptr;
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

}  // namespace

uint64_t BandBatch::order(bool align, size_t row_bytes) { return order_batch(*this, align, row_bytes); }
uint64_t BandDescBatch::order(bool align, size_t row_bytes) { return order_batch(*this, align, row_bytes); }

BandChunk banded_pack_chunk(BandBatch& B, size_t g0, bool align, int ends, const EndsRouting& T) {
    return pack_chunk<true>(B, g0, align, ends, T);
}

BandChunk banded_pack_chunk_tables(BandDescBatch& B, size_t g0, int ends, const EndsRouting& T) {
    return pack_chunk<false>(B, g0, false, ends, T);
}

void banded_host_align(int ends, const uint8_t* q, size_t ql, const uint8_t* d, size_t dl, int64_t lo, int64_t hi,
                       ssa_amd_pair_alignment_t& o, char* text) {
    HostScratch S;
    host_align(ends, q, ql, d, dl, lo, hi, S, o, text);
}

double banded_elapsed(int e) {
    float ms = 0;
    check(hipEventElapsedTime(&ms, g_dev.ev[e], g_dev.ev[e + 1]), "hipEventElapsedTime");
    return (double)ms;
}

int score_pairs_banded(int ends, const int64_t* band_lo, const int64_t* band_hi, const uint8_t* qc,
                       const uint64_t* qoff, const uint8_t* dc, const uint64_t* doff, size_t n, int64_t* scores) {
    const double t0 = now_ms();
    std::vector<int64_t> lo, hi;
    if (!ends_args_ok(ends, qc, qoff, dc, doff, n) || (n && !scores)) return 1;
    if (!bands_ok(ends, band_lo, band_hi, qoff, doff, n, lo, hi)) return 1;
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
    snprintf(S.kernel, sizeof S.kernel, "pairs_banded_i32");

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
            scores[i] = host_score(ends, qc + qoff[i], qoff[i + 1] - qoff[i], dc + doff[i], doff[i + 1] - doff[i],
                                   lo[i], hi[i], W);
        }
    });
    S.host_ms = now_ms() - th0;

    // ---- the device path
    if (!B.idx.empty()) {
        BandedDevice& P = g_dev;
        banded_prepare_device(T.dev_id);
        const double tp0 = now_ms();
        S.swept_cells = B.order(false);
        S.groups = (uint32_t)B.groups.size();
        S.pack_ms += now_ms() - tp0;
        for (size_t g0 = 0; g0 < B.groups.size();) {
            const double tc0 = now_ms();
            const BandChunk K = banded_pack_chunk(B, g0, false, ends, T);
            S.pack_ms += now_ms() - tc0;
            check(hipEventRecord(P.ev[0], T.stream), "hipEventRecord");
            check(launch_pairs_banded(0, K.A, T.stream), "pairs_banded_i32");
            check(hipEventRecord(P.ev[1], T.stream), "hipEventRecord");
            check(hipMemcpyAsync(P.out.h, P.out.d, K.nl * sizeof(int2), hipMemcpyDeviceToHost, T.stream),
                  "pairs_banded scores copy");
            check(hipStreamSynchronize(T.stream), "pairs_banded synchronize");
            S.kernel_ms += banded_elapsed(0);
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

int align_pairs_banded(int ends, const int64_t* band_lo, const int64_t* band_hi, const uint8_t* qc,
                       const uint64_t* qoff, const uint8_t* dc, const uint64_t* doff, size_t n,
                       ssa_amd_pair_alignment_t* out, char* cigars, size_t cigar_cap) {
    const double t0 = now_ms();
    std::vector<int64_t> lo, hi;
    if (!ends_args_ok(ends, qc, qoff, dc, doff, n) || (n && (!out || !cigars))) return 1;
    if (!bands_ok(ends, band_lo, band_hi, qoff, doff, n, lo, hi)) return 1;
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
        // the ends call's conditions, with the direction bits of the band alone: at most 512 MiB for the pair
        if (T.device && ql && dl && (int64_t)(ql + dl) <= T.residue_limit && ql < kAlignMaxLen && dl < kAlignMaxLen &&
            pair_dir_rows(ql, dl, lo[i], hi[i]) * kBandDirRowBytes <= kBandPairDirBudget)
            B.idx.push_back((uint32_t)i);
        else
            todo.push_back(i);
    }
    auto on_host = [&](HostScratch& W, size_t i) {
        out[i].cigar_off = coff[i];
        host_align(ends, qc + qoff[i], qoff[i + 1] - qoff[i], dc + doff[i], doff[i + 1] - doff[i], lo[i], hi[i], W,
                   out[i], cigars + coff[i]);
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
        BandedDevice& P = g_dev;
        banded_prepare_device(T.dev_id);
        snprintf(S.kernels, sizeof S.kernels, "pairs_banded_dir,pairs_banded_walk");
        const double tp0 = now_ms();
        B.order(true);
        S.groups = (uint32_t)B.groups.size();
        S.pack_ms += now_ms() - tp0;
        for (size_t g0 = 0; g0 < B.groups.size();) {
            const double tc0 = now_ms();
            const BandChunk K = banded_pack_chunk(B, g0, true, ends, T);
            S.pack_ms += now_ms() - tc0;
            S.dir_bytes += K.drow * 1024;
            // ---- directions (with the score and the end cell), then the walk from that end cell
            check(hipEventRecord(P.ev[0], T.stream), "hipEventRecord");
            check(launch_pairs_banded(1, K.A, T.stream), "pairs_banded_dir");
            check(hipEventRecord(P.ev[1], T.stream), "hipEventRecord");
            check(launch_pairs_banded(2, K.A, T.stream), "pairs_banded_walk");
            check(hipEventRecord(P.ev[2], T.stream), "hipEventRecord");
            check(hipMemcpyAsync(P.out.h, P.out.d, K.nl * (sizeof(int2) + sizeof(uint32_t)), hipMemcpyDeviceToHost,
                                 T.stream),
                  "pairs_banded results copy");
            if (K.nruns)
                check(hipMemcpyAsync(P.runs.h, P.runs.d, K.nruns * sizeof(uint32_t), hipMemcpyDeviceToHost, T.stream),
                      "pairs_banded runs copy");
            check(hipStreamSynchronize(T.stream), "pairs_banded synchronize");
            S.dir_ms += banded_elapsed(0);
            S.walk_ms += banded_elapsed(1);
            S.launches += 2;

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
                    o.score = h_out[l].x;
                    const uint32_t pos = (uint32_t)h_out[l].y;
                    const uint32_t nr = std::min(h_nruns[l], L.cap);
                    runs.assign(h_runs + L.slot, h_runs + L.slot + nr);
                    o.cigar_len =
                        ends_finish_alignment(ends, pos & 0xffff, pos >> 16, runs, o.region, cigars + coff[i]);
                }
            });
            S.device_fallbacks += lost.load();
            S.host_pairs += lost.load();
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
