// pairs_banded.hip -- the banded pair kernels (layout: pairs_banded.h; host
// side: pairs_banded.cpp).  banded_kernel<DIR> is
// ends_kernel<DIR>'s sweep (pairs_ends.hip: one pair per lane, query rows in
// strips of 8 held in VGPRs, target columns streamed 4 per dword, the lane's
// strip profile in LDS, the bnd row buffer between strips, end maxima kept by
// index) with three changes:
//   * a strip sweeps only the column blocks of its BandStrip, the union of its
//     lanes' in-band columns; a strip with no such block costs nothing, not
//     even its profile;
//   * a cell that does not exist for the lane -- its diagonal k = column - row
//     is outside the lane's own [lo, hi] -- gets H = kBandNegInf, by index;
//   * whatever enters a strip from outside its own cells -- the row above, the
//     column to the left of the first swept one -- is taken by index as well.
// banded_walk_kernel is ends_walk_kernel over the banded direction bits.
//
// Why masking H alone is enough.  E(i, j) is a gap that ends at (i, j) coming
// from the left, F(i, j) one coming from above.  Moving right raises the
// diagonal, moving down lowers it.  A stale E, one that was computed from
// existing cells and then carried past the band's upper edge hi, only moves on
// to greater diagonals; a stale F past the lower edge lo only to smaller ones.
// Neither returns to the band, and on their way they reach H only of cells
// that are masked.  In the other direction, the E that enters the band at its
// lower edge has come along a row of cells left of the band, whose H are all
// kBandNegInf: E = max(E + R, kBandNegInf + Q + R) stays at minus infinity's
// level, provided it STARTED there: column -1 is minus infinity where the
// boundary cell does not exist, and the registers of a strip whose first swept
// column is not column 0 start at kBandNegInf.  The same holds for the F that
// comes down into the band at its upper edge, provided the top row of the
// first strip is minus infinity where its cell does not exist and the (H, F)
// read from bnd are replaced by it where the cell above does not exist.
//
// That last replacement is also what makes bnd safe.  Strip s + 1 sweeps up to
// 8 columns further right than strip s, and the buffer is kept between calls,
// so bnd holds, right of what strip s wrote, plausible finite values of some
// earlier launch.  A lane reads bnd[j] for H(8 s + 7, j) and F.  If that cell
// exists for the lane, j is one of the lane's in-band columns of strip s, so
// strip s swept and wrote it in this launch.  If it does not, the value read is
// discarded by index.  The diagonal entering the first swept column, bnd[4 cb0
// - 1], is covered by the same two cases.
//
// The representative and the bound.  A valid band (pairs_banded.cpp refuses the
// others) makes every in-band cell reachable: going back along its own
// diagonal it meets a boundary cell of that diagonal, which exists.  So every
// existing cell holds a real value, inside +-2^29 by the device score bound
// (ends_route), and minus-infinity-level values live only outside the band and
// in the E / F that arrive from there.  Those are kBandNegInf plus at most one
// gap open and extension or one substitution score, never less: H is reset to
// exactly kBandNegInf wherever it is masked, and E, F >= H + Q + R of a
// neighbour.  All values are therefore in [-2^30 - 512, 2^29]; a real value
// exceeds every minus-infinity-level one by more than 2^29, and push_gt's
// differences are below 2^29 + 2^30 + 512 < 2^31, exact.  The walk only visits
// cells with a real H and reads bits that compare either two real values or a
// real one with minus infinity, so its decisions are the definition's.
//
// Each combination of end tracking and masking is its own straight-line
// instance of block(), as in pairs_ends.hip (see its header's last note); the
// instance without any mask runs in the blocks where all lanes have the 32 cells
// and the 4 cells above them inside their band: there it is ends_kernel's block.
#include "launch.h"
#include "pairs_banded.h"

namespace ssa {
namespace {

constexpr int R = kPairsRows;
constexpr int NEG = kBandNegInf;
static_assert(R == 8, "one uint2 per (code, lane) holds the strip's scores; 32 direction bits per column");

__device__ __forceinline__ int score_of(const uint2 pv, const int r) {
    return (int)(int8_t)((r < 4 ? pv.x : pv.y) >> (8 * (r & 3)));
}

// the lane's strip profile: prof[code][lane] = M[code][rows s*R .. s*R + R) (as ends_kernel)
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

// One column of a strip, as pairs_ends.hip's column().  MASK: row r's cell
// exists iff 0 <= u - r <= span, where u = column - strip's first row - lo is
// the column's diagonal at row 0 of the strip, counted from the band's lower
// edge, and span = hi - lo; the others get H = NEG.
// INT_MAX where 0 <= x <= span, else NEG, in plain arithmetic: as a compare and a select per column the
// four conditions of a block are hoisted and held in SGPR pairs, which costs banded_kernel<true> all 256 VGPRs
__device__ __forceinline__ int cap_of(const int x, const int span) {
    const int bad = (x | (span - x)) >> 31;
    return (bad & NEG) | (~bad & 0x7fffffff);
}

template <bool DIR, bool MASK>
__device__ __forceinline__ uint32_t column(const uint2 pv, int h, int& f, int (&H)[R], int (&E)[R], const int gap_oe,
                                           const int gap_e, const int u, const uint32_t span) {
    uint32_t bits = 0;
#pragma unroll
    for (int r = 0; r < R; r++) {
        const int n = H[r];
        int e = E[r];
        h += score_of(pv, r);
        const bool exists = !MASK || (uint32_t)(u - r) <= span;
        if (!DIR) {
            h = max(h, max(e, f));
            h = exists ? h : NEG;
            H[r] = h;
            const int t = h + gap_oe;
            e = max(e + gap_e, t);
            f = max(f + gap_e, t);
        } else {
            const int d = h;
            const int m = max(d, f);
            h = max(m, e);
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

// What a lane keeps of its end candidates (as pairs_ends.hip).
struct EndTrack {
    int rbest;
    uint32_t rcol;
    int cbest;
    uint32_t crow;
};

// What a lane knows of its own shape and band in this strip.
struct LaneShape {
    uint32_t sel[R];  // ROWCAP: all ones for the lane's last row in its last strip, else 0
    uint32_t rlo;     // ROWCAP: last-row candidates are the columns [rlo, rlo + rcnt)
    uint32_t rcnt;
    uint32_t ccol;    // the lane's last column, dlen - 1
    int rows;         // qlen - s * R: rows r < rows of this strip are real
    int base;         // s * R + lo: column j of the strip has u = j - base
    uint32_t span;    // hi - lo
    bool top_ok;      // first strip: the top row's cells are not ruled out by a missing diagonal 0
    bool left_ok;     // the same for column -1
    int aspan;        // span for the cells ABOVE the strip; -1 (none exists) for a first strip without top_ok
};

// The running state of a strip's sweep between column blocks.
struct Edge {
    int hd;           // H(row0 - 1, j - 1): the diagonal of the next column's top cell
    int top_h, top_f; // the first strip's top boundary by formula: H(-1, j) and the F entering row 0
};

// One block of 4 columns (pairs_ends.hip's block()).  The (H, F) that enter
// from above are taken only where the cell above exists for the lane: that
// cell is (row0 - 1, col), its diagonal counted from lo is u + 1.  Elsewhere
// they become NEG, and what bnd holds there may be anything: clamped from
// below as well, it cannot wrap.  (!MASK: all four cells above exist.)
template <bool DIR, bool ROWCAP, bool COLCAP, bool MASK>
__device__ __forceinline__ uint4 block(const uint2 (&pv)[4], int2 (&b)[4], const bool first, const uint32_t cb,
                                       const uint32_t s, Edge& X, const int top_step, int (&H)[R], int (&E)[R],
                                       EndTrack& T, const LaneShape& L, const int goe, const int Ge) {
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
        dbits[k] = column<DIR, MASK>(pv[k], X.hd, f, H, E, goe, Ge, u, L.span);
        X.hd = th;
        X.top_h += top_step;
        X.top_f += top_step;
        if (ROWCAP) {
            // H of the lane's own last row, selected by mask; a candidate that does not exist holds NEG
            uint32_t hs = 0;
#pragma unroll
            for (int r = 0; r < R; r++) hs |= (uint32_t)H[r] & L.sel[r];
            const bool take = (col - L.rlo < L.rcnt) & ((int)hs >= T.rbest);
            T.rbest = take ? (int)hs : T.rbest;
            T.rcol = take ? col : T.rcol;
        }
        if (COLCAP) {
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

// The swept blocks [S.cb0, S.cb0 + S.ncb) of one strip (S.ncb >= 1).
template <bool DIR, bool ROWCAP>
__device__ __forceinline__ void sweep(const BandedArgs& a, const BandGroup& G, const BandStrip& S, const uint2* prof,
                                      const uint32_t lane, const uint32_t s, const int in_lo, const int in_hi,
                                      int (&H)[R], int (&E)[R], EndTrack& T, const LaneShape& L,
                                      const uint32_t ccb_lo, const uint32_t ccb_span) {
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
        // column -1 (the corner for the first strip): diagonal -(s R), and diagonal 0 unless the q begin is free
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
        if (__builtin_expect(fqe && (DIR || cb - ccb_lo <= ccb_span) && __any(cb == ccb), 0))
            dbits = block<DIR, ROWCAP, true, true>(pv, b, first, cb, s, X, top_step, H, E, T, L, goe, Ge);
        else if ((int)cb >= in_lo && (int)cb <= in_hi)
            dbits = block<DIR, ROWCAP, false, false>(pv, b, first, cb, s, X, top_step, H, E, T, L, goe, Ge);
        else
            dbits = block<DIR, ROWCAP, false, true>(pv, b, first, cb, s, X, top_step, H, E, T, L, goe, Ge);
        if (DIR) dp[(size_t)(cb - cb0) * 64] = dbits;
        if (!last) {
#pragma unroll
            for (int k = 0; k < 4; k++) bp[((size_t)cb * 4 + k) * 64] = b[k];
        }
    }
}

template <bool DIR>
__global__ void __launch_bounds__(64) banded_kernel(const BandedArgs a) {
    __shared__ uint2 prof[kPairsCodes * 64];
    __shared__ uint4 mt[kPairsCodes * 2];
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
    // the lane's last cell (an unused lane, qlen 0, never matches a strip or a column)
    const uint32_t last_strip = (len.x - 1) / R, last_row = (len.x - 1) % R;
    const int Q = a.gap_open, Ge = a.gap_extend, goe = Q + Ge;
    // column -1: H(i, -1) = hq0 + (i + 1) * hq1, both 0 where the q begin is free
    const bool fqb = a.ends & kFreeQBegin, fdb = a.ends & kFreeDBegin;
    const int hq0 = fqb ? 0 : Q, hq1 = fqb ? 0 : Ge;
    // a boundary whose begin is not free is a gap from (-1, -1): it exists only with diagonal 0 in the band
    const bool zero = band.x <= 0 && band.y >= 0;
    EndTrack T;
    T.rbest = T.cbest = (int)0x80000000;
    T.rcol = T.crow = 0;
    LaneShape L;
    L.ccol = len.y - 1;
    L.span = (uint32_t)(band.y - band.x);
    L.top_ok = fdb || zero;
    L.left_ok = fqb || zero;
    // the score kernel: the group's range of last column blocks [ccb_lo, ccb_lo + ccb_span], wave-uniform
    uint32_t ccb_lo = 0, ccb_span = 0xffffffffu;
    if (!DIR) {
        uint32_t blo = len.x ? L.ccol >> 2 : 0xffffffffu, bhi = len.x ? L.ccol >> 2 : 0u;
        for (int o = 32; o; o >>= 1) {
            blo = min(blo, (uint32_t)__shfl_xor((int)blo, o));
            bhi = max(bhi, (uint32_t)__shfl_xor((int)bhi, o));
        }
        ccb_lo = __builtin_amdgcn_readfirstlane(blo);
        ccb_span = __builtin_amdgcn_readfirstlane(bhi) - ccb_lo;
    }
    // the d end not free: the corner is the last row's only candidate
    const uint32_t rlo = (a.ends & kFreeDEnd) ? 0 : len.y - 1;
    for (uint32_t s = 0; s < G.nstrips; s++) {
        const BandStrip S = a.strips[G.s_row + s];
        if (S.ncb == 0) continue;       // no lane has a cell of its band in this strip
        strip_profile(prof, mt, a.qres + (((size_t)G.q_row + 2 * s) * 64 + lane), lane);
        L.base = (int)(s * R) + band.x;
        L.aspan = (s != 0 || L.top_ok) ? (int)L.span : -1;
        // ---- the column left of the first swept one: column -1 where it exists, else nothing exists there
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
        // The blocks [in_lo, in_hi] in which no lane needs a mask: every cell of the block and of the row above
        // it exists -- rows [-1, 8) and columns [0, 4) of block cb have diagonals, counted from lo, in
        // [4 cb - base - 7, 4 cb - base + 4], to lie in [0, aspan].  A lane with no real cell in a block (past
        // its rows, or past its columns from there on) does not care.  One wave reduction per strip.
        int in_lo = (L.base + R - 1 + 3) >> 2, in_hi = (L.aspan + L.base - 4) >> 2;
        if (L.rows <= 0) in_lo = -(1 << 30);
        if (L.rows <= 0 || in_hi + 1 >= (int)((len.y + 3) >> 2)) in_hi = 1 << 30;
        for (int o = 32; o; o >>= 1) {
            in_lo = max(in_lo, __shfl_xor(in_lo, o));
            in_hi = min(in_hi, __shfl_xor(in_hi, o));
        }
        in_lo = __builtin_amdgcn_readfirstlane(in_lo);
        in_hi = __builtin_amdgcn_readfirstlane(in_hi);
        if (__any(mine))
            sweep<DIR, true>(a, G, S, prof, lane, s, in_lo, in_hi, H, E, T, L, ccb_lo, ccb_span);
        else
            sweep<DIR, false>(a, G, S, prof, lane, s, in_lo, in_hi, H, E, T, L, ccb_lo, ccb_span);
    }
    // the rule: the greatest (column, row) among the equal candidates (as ends_kernel)
    const bool row_wins = T.rbest > T.cbest || (T.rbest == T.cbest && T.rcol == len.y - 1);
    const int score = row_wins ? T.rbest : T.cbest;
    const uint32_t col = row_wins ? T.rcol : len.y - 1;
    const uint32_t row = row_wins ? len.x - 1 : T.crow;
    a.out[li] = make_int2(score, (int)(col << 16 | (row & 0xffff)));
}

// The walk, one lane per pair, as ends_walk_kernel.  A cell's bits are found
// through its strip's BandStrip; a walk that stands on a cell outside the
// lane's band or outside the swept blocks loads nothing and reports
// kBandWalkLost (the header says why that is not expected).
__global__ void __launch_bounds__(64) banded_walk_kernel(const BandedArgs a) {
    const uint32_t lane = threadIdx.x;
    const uint32_t g = blockIdx.x;
    const BandGroup G = a.groups[g];
    const size_t li = (size_t)g * 64 + lane;
    const AlignLane L = a.lanes[li];
    uint32_t n = 0;
    if (L.used && L.cap) {
        const uint32_t* dp = (const uint32_t*)a.dir;
        uint32_t* rp = a.runs + L.slot;
        const uint32_t pos = (uint32_t)a.out[li].y;
        int i = (int)(pos & 0xffff), j = (int)(pos >> 16);
        // (an end cell is inside the lane's own pair; anything else walks nowhere)
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

hipError_t launch_pairs_banded(int pass, const BandedArgs& a, hipStream_t st) {
    if (a.ngroups == 0) return hipSuccess;
    const void* k = pass == 0   ? (const void*)&banded_kernel<false>
                    : pass == 1 ? (const void*)&banded_kernel<true>
                                : (const void*)&banded_walk_kernel;
    (void)ssa_launch(k, dim3(a.ngroups), dim3(64), 0, st, a);
    return hipGetLastError();
}

}  // namespace ssa
