// pairs_local.hip -- the local pair kernels (layout: pairs_local.h; host side:
// pairs_local.cpp).  local_kernel<DIR, LB, LE> is
// banded_kernel<DIR>'s sweep (pairs_banded.hip: one pair per lane, query rows
// in strips of 8 held in VGPRs, the swept column blocks of the strip's
// BandStrip, cells outside the lane's band masked to kBandNegInf by index, the
// bnd row buffer between strips) with the two local bits of the mode:
//   * LB, a local begin: H = max(0, D, E, F) in every existing cell, before
//     the band's mask, so a cell outside the band stays minus infinity; the
//     direction pass keeps one more bit per cell, STOP = max(D, E, F) <= 0, in
//     a uint32 per lane and block beside the uint4 of direction bits;
//   * LE, a local end: the candidates are all existing real cells.  Only the
//     score pass (DIR false) tracks them: the greatest H and its position
//     col << 16 | row, strictly greater inside a strip -- columns, and rows
//     inside a column, ascend there -- and "greater, or equal and smaller
//     position" between strips, which is the smallest (d_end, q_end) of the
//     definition.  Candidates are taken BY INDEX (row < qlen, column < dlen):
//     without the floor a padding cell can exceed every real one.  The
//     direction pass under LE tracks nothing and leaves out alone: with the
//     maximum in the same sweep it needs all 256 VGPRs and AGPR copies
//     (DESIGN.md §9.4 has the table), so the end cells come from the
//     score-shaped pass, launched in front of it on the same stream.
//   Without LE the last-row / last-column tracking is banded_kernel's.
// local_walk_kernel is banded_walk_kernel with the STOP test: at a cell it
// stands on through its H (the end cell, after M, or after a gap whose
// extension bit is not set) it first reads STOP and ends there.  Lanes whose
// score is <= 0 walk nowhere: their alignment is empty.
//
// Masking and the bound.  pairs_banded.hip's two arguments hold unchanged.
// The floor replaces a value by 0, which is inside the bound, and a maximum
// creates no new value, so every real value stays inside +-2^29.  E and F need
// no mask of their own with the floor either: they are computed from the H
// that is stored, which is masked AFTER the floor, so a stale E or F that
// leaves the band is still kBandNegInf plus at most one gap, it still only
// moves away from the band, and the floor is applied to H alone -- an E or F
// at minus infinity's level is never raised to 0.  What enters the band from
// outside therefore stays at minus infinity's level, and H >= 0 holds for
// existing cells only.  The STOP bit's difference h - 1 is exact for the same
// reason as push_gt's.
//
// Each combination of tracking and masking is its own straight-line instance
// of block(), masks are arithmetic (cap_of), and there is no branch between
// two columns of a block, as in pairs_banded.hip.
#include "launch.h"
#include "pairs_local.h"

namespace ssa {
namespace {

constexpr int R = kPairsRows;
constexpr int NEG = kBandNegInf;
static_assert(R == 8, "one uint2 per (code, lane) holds the strip's scores; 32 direction bits per column");

__device__ __forceinline__ int score_of(const uint2 pv, const int r) {
    return (int)(int8_t)((r < 4 ? pv.x : pv.y) >> (8 * (r & 3)));
}

// the lane's strip profile: prof[code][lane] = M[code][rows s*R .. s*R + R) (as banded_kernel)
__device__ __forceinline__ void strip_profile(uint2* prof, const uint4* mt, const uint32_t* qp, const uint32_t lane) {
    const uint32_t qw[2] = {qp[0], qp[64]};
#pragma unroll
    for (int half = 0; half < 2; half++) {
        uint32_t v[R][4];
#pragma unroll
        for (int r = 0; r < R; r++) {
            const uint32_t qc = (qw[r >> 2] >> (8 * (r & 3))) & 0xff;
            const uint4 x = mt[qc * 2 + half];
            v[r][0] = x.x;
            v[r][1] = x.y;
            v[r][2] = x.z;
            v[r][3] = x.w;
        }
#pragma unroll
        for (int c = 0; c < 16; c++) {
            const int d = c >> 2, sh = 8 * (c & 3);
            const uint32_t lo = ((v[0][d] >> sh) & 0xff) | (((v[1][d] >> sh) & 0xff) << 8) |
                                (((v[2][d] >> sh) & 0xff) << 16) | (((v[3][d] >> sh) & 0xff) << 24);
            const uint32_t hi = ((v[4][d] >> sh) & 0xff) | (((v[5][d] >> sh) & 0xff) << 8) |
                                (((v[6][d] >> sh) & 0xff) << 16) | (((v[7][d] >> sh) & 0xff) << 24);
            prof[(half * 16 + c) * 64 + lane] = make_uint2(lo, hi);
        }
    }
    prof[kPairsPad * 64 + lane] = make_uint2(0u, 0u);
}

// bits << 1 | (a > b): the sign of b - a shifted in by one v_alignbit (exact: the header's bound)
__device__ __forceinline__ uint32_t push_gt(const uint32_t bits, const int a, const int b) {
    return __builtin_amdgcn_alignbit(bits, (uint32_t)(b - a), 31);
}

// INT_MAX where 0 <= x <= span, else NEG, in plain arithmetic (pairs_banded.hip says why)
__device__ __forceinline__ int cap_of(const int x, const int span) {
    const int bad = (x | (span - x)) >> 31;
    return (bad & NEG) | (~bad & 0x7fffffff);
}

// INT_MAX where x >= 0, else INT_MIN
__device__ __forceinline__ int keep_of(const int x) { return 0x7fffffff ^ (x >> 31); }

// One column of a strip, as pairs_banded.hip's column(); LB: the floor, and in the direction pass the
// cell's STOP bit pushed into stop.
template <bool DIR, bool LB, bool MASK>
__device__ __forceinline__ uint32_t column(const uint2 pv, int h, int& f, int (&H)[R], int (&E)[R], const int gap_oe,
                                           const int gap_e, const int u, const uint32_t span, uint32_t& stop) {
    uint32_t bits = 0;
#pragma unroll
    for (int r = 0; r < R; r++) {
        const int n = H[r];
        int e = E[r];
        h += score_of(pv, r);
        const bool exists = !MASK || (uint32_t)(u - r) <= span;
        if (!DIR) {
            h = max(h, max(e, f));
            if (LB) h = max(h, 0);
            h = exists ? h : NEG;
            H[r] = h;
            const int t = h + gap_oe;
            e = max(e + gap_e, t);
            f = max(f + gap_e, t);
        } else {
            const int d = h;
            const int m = max(d, f);
            h = max(m, e);
            if (LB) {
                stop = __builtin_amdgcn_alignbit(stop, (uint32_t)(h - 1), 31);      // h <= 0
                h = max(h, 0);
            }
            h = exists ? h : NEG;
            H[r] = h;
            const int t = h + gap_oe;
            const int e2 = e + gap_e, f2 = f + gap_e;
            bits = push_gt(bits, e, m);
            bits = push_gt(bits, f, d);
            bits = push_gt(bits, e2, t);
            bits = push_gt(bits, f2, t);
            e = max(e2, t);
            f = max(f2, t);
        }
        E[r] = e;
        h = n;
    }
    return bits;
}

// What a lane keeps of its end candidates: without LE the last row's and the last column's (as
// banded_kernel); with LE the strip's best cell among all of them.
struct EndTrack {
    int rbest;
    uint32_t rcol;
    int cbest;
    uint32_t crow;
    int sbest;
    uint32_t spos;
};

// What a lane knows of its own shape and band in this strip (as banded_kernel).
struct LaneShape {
    uint32_t sel[R];
    uint32_t rlo;
    uint32_t rcnt;
    uint32_t ccol;    // the lane's last column, dlen - 1
    int rows;         // qlen - s * R: rows r < rows of this strip are real
    int base;         // s * R + lo: column j of the strip has u = j - base
    uint32_t span;    // hi - lo
    bool top_ok;
    bool left_ok;
    int aspan;
};

struct Edge {
    int hd;
    int top_h, top_f;
};

// One block of 4 columns (pairs_banded.hip's block()).  ROWCAP / COLCAP without LE: the strip holds a lane's
// last row / the block a lane's last column.  With LE (score pass): the strip holds rows, the block columns,
// past the end of a lane that still has real rows in the strip; a candidate is capped to INT_MIN there.
template <bool DIR, bool LB, bool LE, bool ROWCAP, bool COLCAP, bool MASK>
__device__ __forceinline__ uint4 block(const uint2 (&pv)[4], int2 (&b)[4], const bool first, const uint32_t cb,
                                       const uint32_t s, Edge& X, const int top_step, int (&H)[R], int (&E)[R],
                                       EndTrack& T, const LaneShape& L, const int goe, const int Ge, uint32_t& stop) {
    uint32_t dbits[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const uint32_t col = cb * 4 + k;
        const int u = (int)col - L.base;
        int th = first ? X.top_h : b[k].x;
        int f = first ? X.top_f : b[k].y;
        if (MASK) {
            const int acap = cap_of(u + 1, L.aspan);
            th = max(min(th, acap), NEG);
            f = max(min(f, acap), NEG);
        }
        dbits[k] = column<DIR, LB, MASK>(pv[k], X.hd, f, H, E, goe, Ge, u, L.span, stop);
        X.hd = th;
        X.top_h += top_step;
        X.top_f += top_step;
        if (LE && !DIR) {
            const int ccap = COLCAP ? keep_of((int)L.ccol - (int)col) : 0x7fffffff;
            const uint32_t pos0 = col << 16 | (s * R);
#pragma unroll
            for (int r = 0; r < R; r++) {
                int v = H[r];
                if (COLCAP) v = min(v, ccap);
                if (ROWCAP) v = min(v, keep_of(L.rows - 1 - r));
                const bool take = v > T.sbest;
                T.sbest = take ? v : T.sbest;
                T.spos = take ? pos0 + r : T.spos;
            }
        }
        if (!LE && ROWCAP) {
            uint32_t hs = 0;
#pragma unroll
            for (int r = 0; r < R; r++) hs |= (uint32_t)H[r] & L.sel[r];
            const bool take = (col - L.rlo < L.rcnt) & ((int)hs >= T.rbest);
            T.rbest = take ? (int)hs : T.rbest;
            T.rcol = take ? col : T.rcol;
        }
        if (!LE && COLCAP) {
            const bool here = col == L.ccol;
#pragma unroll
            for (int r = 0; r < R; r++) {
                const bool take = here & (r < L.rows) & (H[r] >= T.cbest);
                T.cbest = take ? H[r] : T.cbest;
                T.crow = take ? s * R + r : T.crow;
            }
        }
        b[k] = make_int2(H[R - 1], f);
    }
    return make_uint4(dbits[0], dbits[1], dbits[2], dbits[3]);
}

// The swept blocks [S.cb0, S.cb0 + S.ncb) of one strip (S.ncb >= 1).  col_min (LE score pass): the smallest
// last column among the lanes with real rows in the strip.
template <bool DIR, bool LB, bool LE, bool ROWCAP>
__device__ __forceinline__ void sweep(const LocalArgs& la, const BandGroup& G, const BandStrip& S, const uint2* prof,
                                      const uint32_t lane, const uint32_t s, const int in_lo, const int in_hi,
                                      int (&H)[R], int (&E)[R], EndTrack& T, const LaneShape& L,
                                      const uint32_t ccb_lo, const uint32_t ccb_span, const uint32_t col_min) {
    const BandedArgs& a = la.b;
    const int Q = a.gap_open, Ge = a.gap_extend, goe = Q + Ge;
    const bool fqb = a.ends & kFreeQBegin, fqe = a.ends & kFreeQEnd, fdb = a.ends & kFreeDBegin;
    const bool first = s == 0, last = s + 1 == G.nstrips;
    const uint32_t* tp = a.tres + ((size_t)G.t_row * 64 + lane);
    int2* bp = a.bnd + ((size_t)G.b_row * 64 + lane);
    const uint32_t cb0 = S.cb0, cb1 = S.cb0 + S.ncb;
    const int top0 = fdb ? 0 : goe, top_step = fdb ? 0 : Ge;
    Edge X;
    X.top_h = top0 + (int)(cb0 * 4) * top_step;
    X.top_f = X.top_h + goe;
    // the diagonal entering the first swept column: H(row0 - 1, 4 cb0 - 1), where that cell exists
    if (cb0 == 0) {
        const bool ex = (uint32_t)(-L.base) <= L.span && (first || L.left_ok);
        X.hd = !ex ? NEG : (first || fqb) ? 0 : Q + (int)(s * R) * Ge;
    } else {
        const int u = (int)(cb0 * 4 - 1) - L.base;
        const bool ex = (uint32_t)(u + 1) <= L.span && (!first || L.top_ok);
        const int v = first ? X.top_h - top_step : bp[(size_t)(cb0 * 4 - 1) * 64].x;
        X.hd = ex ? v : NEG;
    }
    const uint32_t ccb = L.ccol >> 2;
    uint32_t w_next = tp[(size_t)cb0 * 64];
    int2 b_next[4];
#pragma unroll
    for (int k = 0; k < 4; k++) b_next[k] = bp[((size_t)cb0 * 4 + k) * 64];
    uint4* dp = DIR ? a.dir + ((size_t)G.d_row + S.d_off) * 64 + lane : nullptr;
    uint32_t* sp = (DIR && LB) ? la.stop + ((size_t)G.d_row + S.d_off) * 64 + lane : nullptr;
    for (uint32_t cb = cb0; cb < cb1; cb++) {
        const uint32_t w = w_next;
        int2 b[4];
#pragma unroll
        for (int k = 0; k < 4; k++) b[k] = b_next[k];
        // the next block's residues and boundary, in flight during this block's cells
        const uint32_t nb = cb + 1 < cb1 ? cb + 1 : cb;
        w_next = tp[(size_t)nb * 64];
#pragma unroll
        for (int k = 0; k < 4; k++) b_next[k] = bp[((size_t)nb * 4 + k) * 64];
        uint2 pv[4];
#pragma unroll
        for (int k = 0; k < 4; k++) pv[k] = prof[((w >> (8 * k)) & 0xff) * 64 + lane];
        uint4 dbits;
        uint32_t stop = 0;
        bool capped;
        if (LE)
            capped = !DIR && cb * 4 + 3 > col_min;
        else
            capped = fqe && (DIR || cb - ccb_lo <= ccb_span) && __any(cb == ccb);
        if (__builtin_expect(capped, 0))
            dbits = block<DIR, LB, LE, ROWCAP, true, true>(pv, b, first, cb, s, X, top_step, H, E, T, L, goe, Ge, stop);
        else if ((int)cb >= in_lo && (int)cb <= in_hi)
            dbits = block<DIR, LB, LE, ROWCAP, false, false>(pv, b, first, cb, s, X, top_step, H, E, T, L, goe, Ge, stop);
        else
            dbits = block<DIR, LB, LE, ROWCAP, false, true>(pv, b, first, cb, s, X, top_step, H, E, T, L, goe, Ge, stop);
        if (DIR) dp[(size_t)(cb - cb0) * 64] = dbits;
        if (DIR && LB) sp[(size_t)(cb - cb0) * 64] = stop;
        if (!last) {
#pragma unroll
            for (int k = 0; k < 4; k++) bp[((size_t)cb * 4 + k) * 64] = b[k];
        }
    }
}

template <bool DIR, bool LB, bool LE>
__global__ void __launch_bounds__(64) local_kernel(const LocalArgs la) {
    __shared__ uint2 prof[kPairsCodes * 64];
    __shared__ uint4 mt[kPairsCodes * 2];
    const BandedArgs& a = la.b;
    const uint32_t lane = threadIdx.x;
    const uint32_t g = blockIdx.x;
    {
        const uint32_t* src = (const uint32_t*)a.mt;
        uint32_t* dst = (uint32_t*)mt;
        for (uint32_t i = lane; i < kPairsCodes * 8; i += 64) dst[i] = src[i];
    }
    __syncthreads();
    const BandGroup G = a.groups[g];
    const size_t li = (size_t)g * 64 + lane;
    const uint2 len = a.lens[li];
    const int2 band = a.band[li];
    const uint32_t last_strip = (len.x - 1) / R, last_row = (len.x - 1) % R;
    const int Q = a.gap_open, Ge = a.gap_extend, goe = Q + Ge;
    // column -1: H(i, -1) = hq0 + (i + 1) * hq1, both 0 where the q begin is free (a local begin frees both)
    const bool fqb = a.ends & kFreeQBegin, fdb = a.ends & kFreeDBegin;
    const int hq0 = fqb ? 0 : Q, hq1 = fqb ? 0 : Ge;
    const bool zero = band.x <= 0 && band.y >= 0;
    EndTrack T;
    T.rbest = T.cbest = (int)0x80000000;
    T.rcol = T.crow = 0;
    // the best cell of all strips so far (LE score pass)
    int best = (int)0x80000000;
    uint32_t pos = 0xffffffffu;
    LaneShape L;
    L.ccol = len.y - 1;
    L.span = (uint32_t)(band.y - band.x);
    L.top_ok = fdb || zero;
    L.left_ok = fqb || zero;
    // the score kernel without LE: the group's range of last column blocks, wave-uniform
    uint32_t ccb_lo = 0, ccb_span = 0xffffffffu;
    if (!DIR && !LE) {
        uint32_t blo = len.x ? L.ccol >> 2 : 0xffffffffu, bhi = len.x ? L.ccol >> 2 : 0u;
        for (int o = 32; o; o >>= 1) {
            blo = min(blo, (uint32_t)__shfl_xor((int)blo, o));
            bhi = max(bhi, (uint32_t)__shfl_xor((int)bhi, o));
        }
        ccb_lo = __builtin_amdgcn_readfirstlane(blo);
        ccb_span = __builtin_amdgcn_readfirstlane(bhi) - ccb_lo;
    }
    const uint32_t rlo = (a.ends & kFreeDEnd) ? 0 : len.y - 1;
    for (uint32_t s = 0; s < G.nstrips; s++) {
        const BandStrip S = a.strips[G.s_row + s];
        if (S.ncb == 0) continue;       // no lane has a cell of its band in this strip
        strip_profile(prof, mt, a.qres + (((size_t)G.q_row + 2 * s) * 64 + lane), lane);
        L.base = (int)(s * R) + band.x;
        L.aspan = (s != 0 || L.top_ok) ? (int)L.span : -1;
        int H[R], E[R];
        const bool from_edge = S.cb0 == 0 && L.left_ok;
#pragma unroll
        for (int r = 0; r < R; r++) {
            const int i = (int)(s * R) + r;
            const bool ex = from_edge && (uint32_t)(-1 - r - L.base) <= L.span;
            H[r] = ex ? hq0 + (i + 1) * hq1 : NEG;
            E[r] = H[r] + goe;
        }
        L.rows = (int)len.x - (int)(s * R);
        const bool mine = s == last_strip;
#pragma unroll
        for (int r = 0; r < R; r++) L.sel[r] = (mine && last_row == (uint32_t)r) ? 0xffffffffu : 0u;
        L.rlo = rlo;
        L.rcnt = mine ? len.y - rlo : 0;
        // the blocks [in_lo, in_hi] in which no lane needs a band mask (as banded_kernel)
        int in_lo = (L.base + R - 1 + 3) >> 2, in_hi = (L.aspan + L.base - 4) >> 2;
        if (L.rows <= 0) in_lo = -(1 << 30);
        if (L.rows <= 0 || in_hi + 1 >= (int)((len.y + 3) >> 2)) in_hi = 1 << 30;
        // LE score pass: the lanes with real rows here; their smallest last column
        const bool alive = L.rows > 0;
        uint32_t col_min = alive ? L.ccol : 0xffffffffu;
        for (int o = 32; o; o >>= 1) {
            in_lo = max(in_lo, __shfl_xor(in_lo, o));
            in_hi = min(in_hi, __shfl_xor(in_hi, o));
            if (LE && !DIR) col_min = min(col_min, (uint32_t)__shfl_xor((int)col_min, o));
        }
        in_lo = __builtin_amdgcn_readfirstlane(in_lo);
        in_hi = __builtin_amdgcn_readfirstlane(in_hi);
        col_min = __builtin_amdgcn_readfirstlane(col_min);
        T.sbest = (int)0x80000000;
        T.spos = 0xffffffffu;
        const bool rowcap = LE ? (!DIR && __any(alive && L.rows < R)) : __any(mine);
        if (rowcap)
            sweep<DIR, LB, LE, true>(la, G, S, prof, lane, s, in_lo, in_hi, H, E, T, L, ccb_lo, ccb_span, col_min);
        else
            sweep<DIR, LB, LE, false>(la, G, S, prof, lane, s, in_lo, in_hi, H, E, T, L, ccb_lo, ccb_span, col_min);
        if (LE && !DIR) {
            // between strips: greater, or equal and the smaller position (rows grow, columns may not)
            const bool take = alive & ((T.sbest > best) | ((T.sbest == best) & (T.spos < pos)));
            best = take ? T.sbest : best;
            pos = take ? T.spos : pos;
        }
    }
    if (LE) {
        if (!DIR) a.out[li] = make_int2(best, (int)pos);
        return;
    }
    // the rule: the greatest (column, row) among the equal candidates (as banded_kernel)
    const bool row_wins = T.rbest > T.cbest || (T.rbest == T.cbest && T.rcol == len.y - 1);
    const int score = row_wins ? T.rbest : T.cbest;
    const uint32_t col = row_wins ? T.rcol : len.y - 1;
    const uint32_t row = row_wins ? len.x - 1 : T.crow;
    a.out[li] = make_int2(score, (int)(col << 16 | (row & 0xffff)));
}

// The walk, one lane per pair, as banded_walk_kernel, with the STOP test where la.stop is set.
__global__ void __launch_bounds__(64) local_walk_kernel(const LocalArgs la) {
    const BandedArgs& a = la.b;
    const uint32_t lane = threadIdx.x;
    const uint32_t g = blockIdx.x;
    const BandGroup G = a.groups[g];
    const size_t li = (size_t)g * 64 + lane;
    const AlignLane L = a.lanes[li];
    uint32_t n = 0;
    if (L.used && L.cap && a.out[li].x > 0) {
        const uint32_t* dp = (const uint32_t*)a.dir;
        const uint32_t* sp = la.stop;
        uint32_t* rp = a.runs + L.slot;
        const uint32_t pos = (uint32_t)a.out[li].y;
        int i = (int)(pos & 0xffff), j = (int)(pos >> 16);
        const uint2 len = a.lens[li];
        const int2 band = a.band[li];
        const uint32_t span = (uint32_t)(band.y - band.x);
        if ((uint32_t)i >= len.x || (uint32_t)j >= len.y) i = -1;
        uint32_t last = kOpM, op = 3, cnt = 0;
        uint32_t cur = 0xffffffffu;     // the strip S describes
        BandStrip S{};
        bool lost = false;
        while (i >= 0 && j >= 0) {
            const uint32_t s = (uint32_t)i / R;
            if (s != cur) {
                S = a.strips[G.s_row + s];
                cur = s;
            }
            const uint32_t cbk = (uint32_t)j / 4 - S.cb0;
            if ((uint32_t)(j - i - band.x) > span || cbk >= S.ncb) {
                lost = true;
                break;
            }
            const size_t row = (size_t)G.d_row + S.d_off + cbk;
            const uint32_t d = dp[(row * 64 + lane) * 4 + ((uint32_t)j & 3)] >> (4 * (R - 1 - (uint32_t)i % R));
            if (sp) {
                const bool in_gap = (last == kOpI && (d & kDirExtLeft)) || (last == kOpD && (d & kDirExtUp));
                if (!in_gap && ((sp[row * 64 + lane] >> (31 - 8 * ((uint32_t)j & 3) - (uint32_t)i % R)) & 1)) break;
            }
            const uint32_t o = next_op(last, d);
            if (o == op) {
                cnt++;
            } else {
                if (cnt && n < L.cap) rp[n++] = cnt << 2 | op;
                op = o;
                cnt = 1;
            }
            last = o;
            j -= o != kOpD;
            i -= o != kOpI;
        }
        if (cnt && n < L.cap) rp[n++] = cnt << 2 | op;
        if (lost) n = kBandWalkLost;
    }
    a.nruns[li] = n;
}

}  // namespace

hipError_t launch_pairs_local(int pass, int mode, const LocalArgs& a, hipStream_t st) {
    if (a.b.ngroups == 0) return hipSuccess;
    const bool lb = mode & kLocalBegin, le = mode & kLocalEnd;
    const void* k = nullptr;
    if (pass == 0)
        k = lb && le ? (const void*)&local_kernel<false, true, true>
            : lb     ? (const void*)&local_kernel<false, true, false>
                     : (const void*)&local_kernel<false, false, true>;
    else if (pass == 1)
        k = lb && le ? (const void*)&local_kernel<true, true, true>
            : lb     ? (const void*)&local_kernel<true, true, false>
                     : (const void*)&local_kernel<true, false, true>;
    else
        k = (const void*)&local_walk_kernel;
    (void)ssa_launch(k, dim3(a.b.ngroups), dim3(64), 0, st, a);
    return hipGetLastError();
}

}  // namespace ssa
