// pairs_summary.hip -- the summary sweep (layout: pairs_summary.h; host side:
// pairs_summary.cpp).  summary_kernel<LB> is local_kernel's
// score pass (pairs_local.hip: one pair per lane, query rows in strips of 8 held
// in VGPRs, the swept column blocks of the strip's BandStrip, cells outside the
// lane's band masked to kBandNegInf by index, the bnd row buffer between
// strips) without any end tracking -- the end cell is in out, left there by the
// end-cell pass launched in front of it -- and with two words beside every
// value: A = identical << 16 | matched and B = q_begin << 16 | d_begin of the
// path the walk would take back from that value.  The words are selected with
// exactly the comparisons that define the direction bits (pairs_ends.h):
//   H(i, j)   fresh (A = 0, B = (i + 1, j + 1)) under LB where max(D, E, F) <= 0 (STOP);
//             else E's where e > max(d, f) (kDirLeft); else F's where f > d (kDirUp);
//             else the diagonal's, A + 1, and + 0x10000 where the two codes are equal
//   E(i, j+1) E(i, j)'s where e + ge > h + goe with the floored, masked h (kDirExtLeft), else H(i, j)'s
//   F(i+1, j) the same rule with f (kDirExtUp)
// which is next_op read forwards: a gap is followed while its extension bit is
// set, else H decides, left first, then up, then the diagonal; under LB the walk
// stops where it stands on an H with STOP.  So H's words at the end cell are the
// summary of the walk's path, ties included.  Gap columns need no counter: the
// host has columns = q span + d span - matched.  Boundary words are closed
// forms: A = 0; B = (i + 1, 0) at (i, -1) where the q begin is free, (0, j + 1)
// at (-1, j) where the d begin is free, else (0, 0) -- the leading run of a
// begin that is not free then lies inside the spans and counts in columns.
//
// Capture is by index: the lane keeps H's words at (out's row, out's column), in
// the one block() instance with CAP, which runs only in a strip and block where
// some lane ends.  Lanes whose score is <= 0 under a local bit capture nothing.
//
// Masking and the bound.  Values are local_kernel's, so its two arguments hold.
// Words need none of their own: a word is only ever selected together with its
// value, by a strict comparison against the other candidates.  A value at minus
// infinity's level (a cell outside the band, a stale row-buffer entry the cap
// replaced, what leaves the band through E or F) loses every such comparison
// against a real value, so its words -- whatever they are -- reach a real cell
// only where all three candidates are at that level; then H is at that level
// too (no LB), or STOP holds and the words are fresh (LB).  The end cell is a
// real cell with a finite H, so what is captured never came from outside the
// band.  Padding rows and columns lie behind every real cell of their lane in
// both sweep directions and feed none; their counters may wrap, unseen.
// Positions and counters of real cells are below 65 535 (the device condition).
//
// Each combination of capture and masking is its own straight-line instance of
// block(), masks are arithmetic (cap_of), and there is no branch between two
// columns of a block, as in pairs_local.hip.
#include "launch.h"
#include "pairs_summary.h"

namespace ssa {
namespace {

constexpr int R = kPairsRows;
constexpr int NEG = kBandNegInf;
static_assert(R == 8, "one uint2 per (code, lane) holds the strip's scores; two dwords hold its query codes");

__device__ __forceinline__ int score_of(const uint2 pv, const int r) {
    return (int)(int8_t)((r < 4 ? pv.x : pv.y) >> (8 * (r & 3)));
}

// the lane's strip profile: prof[code][lane] = M[code][rows s*R .. s*R + R) (as local_kernel)
__device__ __forceinline__ void strip_profile(uint2* prof, const uint4* mt, const uint32_t (&qw)[2], const uint32_t lane) {
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

// INT_MAX where 0 <= x <= span, else NEG, in plain arithmetic (pairs_banded.hip says why)
__device__ __forceinline__ int cap_of(const int x, const int span) {
    const int bad = (x | (span - x)) >> 31;
    return (bad & NEG) | (~bad & 0x7fffffff);
}

// Bit 8 b + 7 set where byte b of the four query codes equals the column's code (codes are below 64, so
// no carry leaves a byte).
__device__ __forceinline__ uint32_t equal_bytes(const uint32_t qw, const uint32_t code) {
    return (((qw ^ (code * 0x01010101u)) + 0x7f7f7f7fu) & 0x80808080u) ^ 0x80808080u;
}

// The strip's values and their words: H and E of the 8 rows.
struct Strip {
    int H[R], E[R];
    uint32_t HA[R], HB[R], EA[R], EB[R];
};

// A value entering a column from above or from the diagonal, with its words.
struct Cell {
    int v;
    uint32_t a, b;
};

// One column of a strip: local_kernel's score column with the words.  eq: equal_bytes of the strip's two
// code dwords; fresh: B of a path that begins in row 0 of the strip at this column.
template <bool LB, bool MASK>
__device__ __forceinline__ void column(const uint2 pv, const uint32_t (&eq)[2], Cell h, Cell& f, Strip& W,
                                       const int gap_oe, const int gap_e, const int u, const uint32_t span,
                                       const uint32_t fresh) {
#pragma unroll
    for (int r = 0; r < R; r++) {
        const Cell n = {W.H[r], W.HA[r], W.HB[r]};
        const int e = W.E[r];
        const int d = h.v + score_of(pv, r);
        const int m = max(d, f.v);
        int hv = max(m, e);
        const bool left = e > m, up = f.v > d;
        uint32_t a = h.a + 1 + (((eq[r >> 2] >> (8 * (r & 3) + 7)) & 1) << 16), b = h.b;
        a = up ? f.a : a;
        b = up ? f.b : b;
        a = left ? W.EA[r] : a;
        b = left ? W.EB[r] : b;
        if (LB) {
            const bool stop = hv <= 0;
            a = stop ? 0u : a;
            b = stop ? fresh + ((uint32_t)r << 16) : b;
            hv = max(hv, 0);
        }
        const bool exists = !MASK || (uint32_t)(u - r) <= span;
        hv = exists ? hv : NEG;
        W.H[r] = hv;
        W.HA[r] = a;
        W.HB[r] = b;
        const int t = hv + gap_oe;
        const int e2 = e + gap_e, f2 = f.v + gap_e;
        const bool ext_left = e2 > t, ext_up = f2 > t;
        W.EA[r] = ext_left ? W.EA[r] : a;
        W.EB[r] = ext_left ? W.EB[r] : b;
        f.a = ext_up ? f.a : a;
        f.b = ext_up ? f.b : b;
        W.E[r] = max(e2, t);
        f.v = max(f2, t);
        h = n;
    }
}

// What a lane knows of its own shape, band and end cell in this strip.
struct LaneShape {
    int base;         // s * R + lo: column j of the strip has u = j - base
    uint32_t span;    // hi - lo
    bool top_ok;
    bool left_ok;
    int aspan;
    uint32_t top_b;   // 1 where the d begin is free: B of (-1, j) is top_b * (j + 1)
    bool mine;        // the lane's end cell lies in this strip
    uint32_t erow;    // ... in this row of it
    uint32_t ecol;    // ... in this column
};

struct Edge {
    Cell hd;          // the diagonal entering the next column's row 0
    int top_h, top_f; // row -1's H and F of the next column (first strip)
};

// One block of 4 columns (pairs_local.hip's block()).  CAP: some lane's end cell lies in this block of this
// strip; the lane takes H's words there, by index.
template <bool LB, bool CAP, bool MASK>
__device__ __forceinline__ void block(const uint2 (&pv)[4], const uint32_t w, const uint32_t (&qw)[2], int2 (&b)[4],
                                      uint4 (&bw)[4], const bool first, const uint32_t cb, const uint32_t s, Edge& X,
                                      const int top_step, Strip& W, const LaneShape& L, const int goe, const int Ge,
                                      uint2& cap) {
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const uint32_t col = cb * 4 + k;
        const int u = (int)col - L.base;
        const uint32_t tb = L.top_b * (col + 1);
        Cell th = {first ? X.top_h : b[k].x, first ? 0u : bw[k].x, first ? tb : bw[k].y};
        Cell f = {first ? X.top_f : b[k].y, first ? 0u : bw[k].z, first ? tb : bw[k].w};
        if (MASK) {
            const int acap = cap_of(u + 1, L.aspan);
            th.v = max(min(th.v, acap), NEG);
            f.v = max(min(f.v, acap), NEG);
        }
        const uint32_t code = (w >> (8 * k)) & 0xff;
        const uint32_t eq[2] = {equal_bytes(qw[0], code), equal_bytes(qw[1], code)};
        column<LB, MASK>(pv[k], eq, X.hd, f, W, goe, Ge, u, L.span, ((s * R + 1) << 16) | (col + 1));
        X.hd = th;
        X.top_h += top_step;
        X.top_f += top_step;
        if (CAP) {
            const bool here = L.mine & (col == L.ecol);
#pragma unroll
            for (int r = 0; r < R; r++) {
                const bool take = here & (L.erow == (uint32_t)r);
                cap.x = take ? W.HA[r] : cap.x;
                cap.y = take ? W.HB[r] : cap.y;
            }
        }
        b[k] = make_int2(W.H[R - 1], f.v);
        bw[k] = make_uint4(W.HA[R - 1], W.HB[R - 1], f.a, f.b);
    }
}

// The swept blocks [S.cb0, S.cb0 + S.ncb) of one strip (S.ncb >= 1).  any_mine: some lane ends in the strip.
template <bool LB>
__device__ __forceinline__ void sweep(const SummaryArgs& sa, const BandGroup& G, const BandStrip& S, const uint2* prof,
                                      const uint32_t (&qw)[2], const uint32_t lane, const uint32_t s, const int in_lo,
                                      const int in_hi, Strip& W, const LaneShape& L, const bool any_mine, uint2& cap) {
    const BandedArgs& a = sa.b;
    const int Q = a.gap_open, Ge = a.gap_extend, goe = Q + Ge;
    const bool fqb = a.ends & kFreeQBegin, fdb = a.ends & kFreeDBegin;
    const bool first = s == 0, last = s + 1 == G.nstrips;
    const uint32_t* tp = a.tres + ((size_t)G.t_row * 64 + lane);
    int2* bp = a.bnd + ((size_t)G.b_row * 64 + lane);
    uint4* wp = sa.rows + ((size_t)G.b_row * 64 + lane);
    const uint32_t cb0 = S.cb0, cb1 = S.cb0 + S.ncb;
    const int top0 = fdb ? 0 : goe, top_step = fdb ? 0 : Ge;
    Edge X;
    X.top_h = top0 + (int)(cb0 * 4) * top_step;
    X.top_f = X.top_h + goe;
    // the diagonal entering the first swept column: H(row0 - 1, 4 cb0 - 1), where that cell exists
    if (cb0 == 0) {
        const bool ex = (uint32_t)(-L.base) <= L.span && (first || L.left_ok);
        X.hd.v = !ex ? NEG : (first || fqb) ? 0 : Q + (int)(s * R) * Ge;
        X.hd.a = 0;
        X.hd.b = (!first && fqb) ? (s * R) << 16 : 0u;
    } else {
        const int u = (int)(cb0 * 4 - 1) - L.base;
        const bool ex = (uint32_t)(u + 1) <= L.span && (!first || L.top_ok);
        const size_t at = (size_t)(cb0 * 4 - 1) * 64;
        const int v = first ? X.top_h - top_step : bp[at].x;
        X.hd.v = ex ? v : NEG;
        X.hd.a = first ? 0u : wp[at].x;
        X.hd.b = first ? L.top_b * (cb0 * 4) : wp[at].y;
    }
    const uint32_t ecb = L.ecol >> 2;
    uint32_t w_next = tp[(size_t)cb0 * 64];
    int2 b_next[4];
    uint4 bw_next[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        b_next[k] = bp[((size_t)cb0 * 4 + k) * 64];
        bw_next[k] = wp[((size_t)cb0 * 4 + k) * 64];
    }
    for (uint32_t cb = cb0; cb < cb1; cb++) {
        const uint32_t w = w_next;
        int2 b[4];
        uint4 bw[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            b[k] = b_next[k];
            bw[k] = bw_next[k];
        }
        // the next block's residues and boundary, in flight during this block's cells
        const uint32_t nb = cb + 1 < cb1 ? cb + 1 : cb;
        w_next = tp[(size_t)nb * 64];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            b_next[k] = bp[((size_t)nb * 4 + k) * 64];
            bw_next[k] = wp[((size_t)nb * 4 + k) * 64];
        }
        uint2 pv[4];
#pragma unroll
        for (int k = 0; k < 4; k++) pv[k] = prof[((w >> (8 * k)) & 0xff) * 64 + lane];
        const bool capped = any_mine && __any(L.mine & (cb == ecb));
        if (__builtin_expect(capped, 0))
            block<LB, true, true>(pv, w, qw, b, bw, first, cb, s, X, top_step, W, L, goe, Ge, cap);
        else if ((int)cb >= in_lo && (int)cb <= in_hi)
            block<LB, false, false>(pv, w, qw, b, bw, first, cb, s, X, top_step, W, L, goe, Ge, cap);
        else
            block<LB, false, true>(pv, w, qw, b, bw, first, cb, s, X, top_step, W, L, goe, Ge, cap);
        if (!last) {
#pragma unroll
            for (int k = 0; k < 4; k++) {
                bp[((size_t)cb * 4 + k) * 64] = b[k];
                wp[((size_t)cb * 4 + k) * 64] = bw[k];
            }
        }
    }
}

template <bool LB>
__global__ void __launch_bounds__(64) summary_kernel(const SummaryArgs sa, const int local) {
    __shared__ uint2 prof[kPairsCodes * 64];
    __shared__ uint4 mt[kPairsCodes * 2];
    const BandedArgs& a = sa.b;
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
    const int2 end = a.out[li];
    const int Q = a.gap_open, Ge = a.gap_extend, goe = Q + Ge;
    // column -1: H(i, -1) = hq0 + (i + 1) * hq1, both 0 where the q begin is free (a local begin frees both)
    const bool fqb = a.ends & kFreeQBegin, fdb = a.ends & kFreeDBegin;
    const int hq0 = fqb ? 0 : Q, hq1 = fqb ? 0 : Ge;
    const bool zero = band.x <= 0 && band.y >= 0;
    // the end cell, from the pass in front; a lane without one (unused, or the empty alignment) captures nothing
    const uint32_t erow = (uint32_t)end.y & 0xffff, ecol = (uint32_t)end.y >> 16;
    const bool want = erow < len.x && ecol < len.y && (!local || end.x > 0);
    LaneShape L;
    L.span = (uint32_t)(band.y - band.x);
    L.top_ok = fdb || zero;
    L.left_ok = fqb || zero;
    L.top_b = fdb ? 1u : 0u;
    L.erow = erow % R;
    L.ecol = ecol;
    uint2 cap = make_uint2(0u, 0u);
    for (uint32_t s = 0; s < G.nstrips; s++) {
        const BandStrip S = a.strips[G.s_row + s];
        if (S.ncb == 0) continue;       // no lane has a cell of its band in this strip
        const uint32_t* qp = a.qres + (((size_t)G.q_row + 2 * s) * 64 + lane);
        const uint32_t qw[2] = {qp[0], qp[64]};
        strip_profile(prof, mt, qw, lane);
        L.base = (int)(s * R) + band.x;
        L.aspan = (s != 0 || L.top_ok) ? (int)L.span : -1;
        Strip W;
        const bool from_edge = S.cb0 == 0 && L.left_ok;
#pragma unroll
        for (int r = 0; r < R; r++) {
            const int i = (int)(s * R) + r;
            const bool ex = from_edge && (uint32_t)(-1 - r - L.base) <= L.span;
            W.H[r] = ex ? hq0 + (i + 1) * hq1 : NEG;
            W.E[r] = W.H[r] + goe;
            W.HA[r] = W.EA[r] = 0;
            W.HB[r] = W.EB[r] = fqb ? (uint32_t)(i + 1) << 16 : 0u;
        }
        const int rows = (int)len.x - (int)(s * R);
        L.mine = want && erow / R == s;
        // the blocks [in_lo, in_hi] in which no lane needs a band mask (as local_kernel)
        int in_lo = (L.base + R - 1 + 3) >> 2, in_hi = (L.aspan + L.base - 4) >> 2;
        if (rows <= 0) in_lo = -(1 << 30);
        if (rows <= 0 || in_hi + 1 >= (int)((len.y + 3) >> 2)) in_hi = 1 << 30;
        for (int o = 32; o; o >>= 1) {
            in_lo = max(in_lo, __shfl_xor(in_lo, o));
            in_hi = min(in_hi, __shfl_xor(in_hi, o));
        }
        in_lo = __builtin_amdgcn_readfirstlane(in_lo);
        in_hi = __builtin_amdgcn_readfirstlane(in_hi);
        sweep<LB>(sa, G, S, prof, qw, lane, s, in_lo, in_hi, W, L, __any(L.mine), cap);
    }
    sa.sum[li] = cap;
}

}  // namespace

hipError_t launch_pairs_summary(bool lb, bool local, const SummaryArgs& a, hipStream_t st) {
    if (a.b.ngroups == 0) return hipSuccess;
    const void* k = lb ? (const void*)&summary_kernel<true> : (const void*)&summary_kernel<false>;
    const int loc = local;
    (void)ssa_launch(k, dim3(a.b.ngroups), dim3(64), 0, st, a, loc);
    return hipGetLastError();
}

}  // namespace ssa
