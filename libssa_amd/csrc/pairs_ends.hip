// pairs_ends.hip -- the ends-free (semi-global) pair kernels (layout:
// pairs_ends.h; host side: pairs_ends.cpp).  ends_kernel<DIR>
// is pairs_kernel<true>'s sweep (DIR: with direction bits per cell, as
// sweep_kernel<DIR_NW>) with the mask `ends` as a wave-uniform argument:
//   * a free BEGIN is a zero boundary: scalar values and scalar increments of
//     the first strip's top row, of each strip's column -1 and of the diagonal
//     entering column 0;
//   * a free END is a maximum over the lane's own last column and / or last
//     row, kept with its position; the corner is always a candidate.
// ends_walk_kernel then follows the bits from the end cell.
// The conventions are pairs.hip's: one pair per lane, query rows in strips of
// 8 held in VGPRs, target columns streamed 4 per dword, the lane's strip
// profile in LDS, the bnd row buffer between strips, padding code 32.
//
// Why the end maxima are exact although shorter lanes are masked by value.
// (1) A cell (i, j) reads only cells (i', j') with i' <= i and j' <= j and the
// boundaries, so H, E, F and the direction bits of a REAL cell (i < qlen and
// j < dlen) never depend on a padding cell: they are the lane's own pair's,
// whatever the group sweeps beyond it.  (2) Padding cells, unlike SW's and
// NW's, must stay out of the maxima -- a padding cell scores 0 against
// everything and can exceed every real candidate, with gap penalties of 0 it
// simply repeats its neighbour -- and no value argument keeps them out.  They
// are kept out BY INDEX: a last-column candidate is taken only at the lane's
// own column dlen - 1 and at rows < qlen, a last-row candidate only from row
// qlen - 1 of the lane's own last strip and at columns < dlen (only at column
// dlen - 1 when the d end is not free).  Every candidate is therefore a real
// cell of the definition's candidate set, and every cell of that set is
// visited once, so by (1) the maximum is the definition's.  (3) Ties: last-row
// candidates arrive by ascending column and last-column candidates by
// ascending (strip, row), each replacing the kept one when >=, so each set
// keeps its greatest position; the two are combined by the rule (greatest
// (column, row)) after the sweep.
//
// The index tests cost next to nothing where no lane ends: the last-row code
// runs in strips where __any(lane's last strip), the last-column code in
// column blocks where __any(lane's last block); both tests are wave-uniform,
// no lane branches on its own lengths.  Each combination is its own
// straight-line instance of block(): a branch between two columns of a block
// costs the DIR kernel all 256 VGPRs (it sits at 164 of the 168 that keep 3
// waves per SIMD, and small changes of the sweep's shape tip it over: check
// -Rpass-analysis=kernel-resource-usage after any edit).
#include "launch.h"
#include "pairs_ends.h"

namespace ssa {
namespace {

constexpr int R = kPairsRows;
static_assert(R == 8, "one uint2 per (code, lane) holds the strip's scores; 32 direction bits per column");

__device__ __forceinline__ int score_of(const uint2 pv, const int r) {
    return (int)(int8_t)((r < 4 ? pv.x : pv.y) >> (8 * (r & 3)));
}

// the lane's strip profile: prof[code][lane] = M[code][rows s*R .. s*R + R) (as pairs_kernel)
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

// bits << 1 | (a > b): the sign of b - a shifted in by one v_alignbit (the
// values are inside 2^29, pairs_ends.cpp's routing, so the difference is exact)
__device__ __forceinline__ uint32_t push_gt(const uint32_t bits, const int a, const int b) {
    return __builtin_amdgcn_alignbit(bits, (uint32_t)(b - a), 31);
}

// One column of a strip: h enters as the diagonal H(row0 - 1, j - 1), f as the
// F coming down from the strip above; H[r] / E[r] hold column j - 1 on entry
// and column j on exit.  DIR: returns the column's direction bits, four per
// cell, derived exactly as directions() (align.cpp) derives them for NW:
//   LEFT      H took e (after the diagonal and f)      UP      H took f (after the diagonal)
//   EXT_LEFT  the next column's E extends this E       EXT_UP  the next row's F extends this F
// Each bit is shifted in from the right, so row r's nibble ends at bits
// 4 * (7 - r), LEFT = 8, UP = 4, EXT_LEFT = 2, EXT_UP = 1 inside it (pairs_ends.h).
template <bool DIR>
__device__ __forceinline__ uint32_t column(const uint2 pv, int h, int& f, int (&H)[R], int (&E)[R], const int gap_oe,
                                           const int gap_e) {
    uint32_t bits = 0;
#pragma unroll
    for (int r = 0; r < R; r++) {
        const int n = H[r];
        int e = E[r];
        h += score_of(pv, r);
        if (!DIR) {
            h = max(h, max(e, f));
            H[r] = h;
            const int t = h + gap_oe;
            e = max(e + gap_e, t);
            f = max(f + gap_e, t);
        } else {
            const int d = h;
            const int m = max(d, f);
            h = max(m, e);
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

// What a lane keeps of its end candidates.
struct EndTrack {
    int rbest;        // last row (qlen - 1): the maximum over its candidate columns
    uint32_t rcol;    //   and the greatest column that holds it
    int cbest;        // last column (dlen - 1), FREE_Q_END only: the maximum over rows < qlen
    uint32_t crow;    //   and the greatest row that holds it
};

// What a lane knows of its own shape in this strip.
struct LaneShape {
    uint32_t sel[R];  // ROWCAP: all ones for the lane's last row in its last strip, else 0
    uint32_t rlo;     // ROWCAP: last-row candidates are the columns [rlo, rlo + rcnt)
    uint32_t rcnt;    //   (rcnt 0: this is not the lane's last strip)
    uint32_t ccol;    // the lane's last column, dlen - 1
    int rows;         // qlen - s * R: rows r < rows of this strip are real
};

// The running state of a strip's sweep between column blocks.
struct Edge {
    int hd;           // H(row0 - 1, j - 1): the diagonal of the next column's top cell
    int top_h, top_f; // the first strip's top boundary by formula: H(-1, j) and the F entering row 0
};

// One block of 4 columns.  ROWCAP: some lane's last row lies in this strip;
// COLCAP: some lane's last column lies in this block.  Both are template
// arguments so that a block is straight-line code (the header's last note).
template <bool DIR, bool ROWCAP, bool COLCAP>
__device__ __forceinline__ uint4 block(const uint2 (&pv)[4], int2 (&b)[4], const bool first, const uint32_t cb,
                                       const uint32_t s, Edge& X, const int top_step, int (&H)[R],
                                       int (&E)[R], EndTrack& T, const LaneShape& L, const int goe, const int Ge) {
    uint32_t dbits[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const uint32_t col = cb * 4 + k;
        const int th = first ? X.top_h : b[k].x;
        int f = first ? X.top_f : b[k].y;
        dbits[k] = column<DIR>(pv[k], X.hd, f, H, E, goe, Ge);
        X.hd = th;
        X.top_h += top_step;
        X.top_f += top_step;
        if (ROWCAP) {
            // H of the lane's own last row, selected by mask (as pairs_kernel's CAP)
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

// All columns of one strip.
template <bool DIR, bool ROWCAP>
__device__ __forceinline__ void sweep(const EndsArgs& a, const AlignGroup& G, const uint2* prof, const uint32_t lane,
                                      const uint32_t s, int (&H)[R], int (&E)[R], EndTrack& T, const LaneShape& L,
                                      const uint32_t ccb_lo, const uint32_t ccb_span) {
    const int Q = a.gap_open, Ge = a.gap_extend, goe = Q + Ge;
    const bool fqb = a.ends & kFreeQBegin, fqe = a.ends & kFreeQEnd, fdb = a.ends & kFreeDBegin;
    const bool first = s == 0, last = s + 1 == G.nstrips;
    const uint32_t* tp = a.tres + ((size_t)G.t_row * 64 + lane);
    int2* bp = a.bnd + ((size_t)G.b_row * 64 + lane);
    Edge X;
    X.hd = (first || fqb) ? 0 : Q + (int)(s * R) * Ge;
    const int top0 = fdb ? 0 : goe, top_step = fdb ? 0 : Ge;
    X.top_h = top0;
    X.top_f = top0 + goe;
    const uint32_t ccb = L.ccol >> 2;
    uint32_t w_next = tp[0];
    int2 b_next[4];
#pragma unroll
    for (int k = 0; k < 4; k++) b_next[k] = bp[(size_t)k * 64];
    for (uint32_t cb = 0; cb < G.ncb; cb++) {
        const uint32_t w = w_next;
        int2 b[4];
#pragma unroll
        for (int k = 0; k < 4; k++) b[k] = b_next[k];
        // the next block's residues and boundary, in flight during this block's cells
        const uint32_t nb = cb + 1 < G.ncb ? cb + 1 : cb;
        w_next = tp[(size_t)nb * 64];
#pragma unroll
        for (int k = 0; k < 4; k++) b_next[k] = bp[((size_t)nb * 4 + k) * 64];
        uint2 pv[4];
#pragma unroll
        for (int k = 0; k < 4; k++) pv[k] = prof[((w >> (8 * k)) & 0xff) * 64 + lane];
        // some lane's last column lies in this block (the score kernel asks only inside the group's range of
        // last blocks, with scalar compares: batches are shape-sorted, so the range is narrow)
        uint4 dbits;
        if (__builtin_expect(fqe && (DIR || cb - ccb_lo <= ccb_span) && __any(cb == ccb), 0))
            dbits = block<DIR, ROWCAP, true>(pv, b, first, cb, s, X, top_step, H, E, T, L, goe, Ge);
        else
            dbits = block<DIR, ROWCAP, false>(pv, b, first, cb, s, X, top_step, H, E, T, L, goe, Ge);
        if (DIR) a.dir[((size_t)G.d_row + (size_t)s * G.ncb + cb) * 64 + lane] = dbits;
        if (!last) {
#pragma unroll
            for (int k = 0; k < 4; k++) bp[((size_t)cb * 4 + k) * 64] = b[k];
        }
    }
}

template <bool DIR>
__global__ void __launch_bounds__(64) ends_kernel(const EndsArgs a) {
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
    const AlignGroup G = a.groups[g];
    const size_t li = (size_t)g * 64 + lane;
    const uint2 len = a.lens[li];
    // the lane's last cell (an unused lane, qlen 0, never matches a strip or a column)
    const uint32_t last_strip = (len.x - 1) / R, last_row = (len.x - 1) % R;
    const int Q = a.gap_open, Ge = a.gap_extend, goe = Q + Ge;
    // column -1: H(i, -1) = hq0 + (i + 1) * hq1, both 0 where the q begin is free
    const bool fqb = a.ends & kFreeQBegin;
    const int hq0 = fqb ? 0 : Q, hq1 = fqb ? 0 : Ge;
    EndTrack T;
    T.rbest = T.cbest = (int)0x80000000;
    T.rcol = T.crow = 0;
    LaneShape L;
    L.ccol = len.y - 1;
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
        strip_profile(prof, mt, a.qres + (((size_t)G.q_row + 2 * s) * 64 + lane), lane);
        // ---- column -1 of the strip
        int H[R], E[R];
#pragma unroll
        for (int r = 0; r < R; r++) {
            const int i = (int)(s * R) + r;
            H[r] = hq0 + (i + 1) * hq1;
            E[r] = H[r] + goe;
        }
        L.rows = (int)len.x - (int)(s * R);
        const bool mine = s == last_strip;
#pragma unroll
        for (int r = 0; r < R; r++) L.sel[r] = (mine && last_row == (uint32_t)r) ? 0xffffffffu : 0u;
        L.rlo = rlo;
        L.rcnt = mine ? len.y - rlo : 0;
        if (__any(mine))
            sweep<DIR, true>(a, G, prof, lane, s, H, E, T, L, ccb_lo, ccb_span);
        else
            sweep<DIR, false>(a, G, prof, lane, s, H, E, T, L, ccb_lo, ccb_span);
    }
    // the rule: the greatest (column, row) among the equal candidates.  The kept last-column cell has the
    // greatest column there is, so the last row's wins a tie only as the corner.
    const bool row_wins = T.rbest > T.cbest || (T.rbest == T.cbest && T.rcol == len.y - 1);
    const int score = row_wins ? T.rbest : T.cbest;
    const uint32_t col = row_wins ? T.rcol : len.y - 1;
    const uint32_t row = row_wins ? len.x - 1 : T.crow;
    a.out[li] = make_int2(score, (int)(col << 16 | (row & 0xffff)));
}

// The walk, one lane per pair, from the end cell ends_kernel<true> left in out
// until it leaves the matrix: cigar()'s order (align.cpp) -- left ('I', along
// the target) first, then up ('D', along the query), else diagonal ('M') --
// with the state an affine gap needs.  A cell entered through a gap reads its
// extension bit first: EXT_LEFT of (i, j) says that E of column j + 1 extends
// E(i, j), so a walk that came from (i, j + 1) by 'I' goes on to the left;
// without the bit that gap opened from H(i, j), and LEFT / UP say where H(i, j)
// came from.  (cigar() reads the extension bits whichever way it entered a
// cell; its text then need not re-score to the score.)  Each step is one
// dependent 4-byte load of the lane's own direction bits; runs are
// walk_kernel's: count << 2 | op in traceback order.
__global__ void __launch_bounds__(64) ends_walk_kernel(const EndsArgs a) {
    const uint32_t lane = threadIdx.x;
    const uint32_t g = blockIdx.x;
    const AlignGroup G = a.groups[g];
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
        if ((uint32_t)i >= len.x || (uint32_t)j >= len.y) i = -1;
        uint32_t last = kOpM, op = 3, cnt = 0;
        while (i >= 0 && j >= 0) {
            const size_t row = (size_t)G.d_row + (size_t)((uint32_t)i / R) * G.ncb + (uint32_t)j / 4;
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
    }
    a.nruns[li] = n;
}

}  // namespace

hipError_t launch_pairs_ends(int pass, const EndsArgs& a, hipStream_t st) {
    if (a.ngroups == 0) return hipSuccess;
    const void* k = pass == 0   ? (const void*)&ends_kernel<false>
                    : pass == 1 ? (const void*)&ends_kernel<true>
                                : (const void*)&ends_walk_kernel;
    (void)ssa_launch(k, dim3(a.ngroups), dim3(64), 0, st, a);
    return hipGetLastError();
}

}  // namespace ssa
