// pairs_align.hip -- the batch aligner's kernels (layout: pairs_align.h; host
// side: pairs_align.cpp).  The conventions are pairs.hip's:
// one pair per lane, query rows in strips of 8 held in VGPRs, target columns
// streamed 4 per dword, the lane's strip profile in LDS, the bnd row buffer
// between strips, padding code 32.  sweep_kernel<MODE> is that sweep with
// what the reference's traceback (align.cpp) needs of it:
//   FWD     SW forward: the maximum and the first cell that holds it in the
//           reference's order (target index outer, query index inner), and
//           every row's (H, E) after the lane's last column (fin)
//   REV     SW reverse from the end cell, no floor: the first cell that
//           reaches the maximum
//   DIR_SW / DIR_NW   two direction bits per cell (and NW's score)
// walk_kernel then follows the bits from the end cell and writes the
// alignment as runs.
//
// FWD needs no mask on its candidates.  A padding cell (row >= qlen or column
// >= dlen) scores 0 against everything, so its H is max(diagonal H, e, f, 0)
// and, gap penalties being <= 0 (pairs_align.cpp sends anything else to the
// host), e and f are at most an H to its left / above it.  By induction over
// row + column, H of a padding cell (i, j) is at most max(0, H of the real
// cells (i', j') with i' <= i and j' <= j).  Each of those real cells comes
// before (i, j) in (column, row) order, and a candidate replaces the kept one
// only when it is greater, or equal and earlier in that order.  So a padding
// cell can take the maximum only at 0, which is a zero pair whatever the
// position.  Nothing here needs a penalty to be strictly negative: with
// gap_open = gap_extend = 0 every "at most" above still holds as written.
#include "launch.h"
#include "pairs_align.h"

namespace ssa {
namespace {

constexpr int R = kPairsRows;
static_assert(R == 8, "one uint2 per (code, lane) holds the strip's scores; 16 direction bits per column");

enum Mode { FWD = 0, REV = 1, DIR_SW = 2, DIR_NW = 3 };

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

// What a sweep keeps per lane besides H / E.
struct Track {
    int sb;               // FWD: the strip's maximum
    uint32_t sp;          // FWD: its first cell; REV: the first cell that reaches thr (minimum of col << 16 | row)
    int thr[R];           // REV: the score to reach, INT_MAX on rows outside the lane's rectangle
};

// One column of a strip: h enters as the diagonal H(row0 - 1, j - 1), f as the
// F coming down from the strip above; H[r] / E[r] hold column j - 1 on entry
// and column j on exit.  cpos = col << 16 | row0 (REV: 0xffff in the column
// half when the column is outside the lane's rectangle).  Returns the column's
// 16 direction bits (DIR modes).
template <int MODE>
__device__ __forceinline__ uint32_t column(const uint2 pv, int h, int& f, int (&H)[R], int (&E)[R], Track& T,
                                           const uint32_t cpos, const int gap_oe, const int gap_e) {
    uint32_t bits = 0;
#pragma unroll
    for (int r = 0; r < R; r++) {
        const int n = H[r];
        int e = E[r];
        h += score_of(pv, r);
        if (MODE == FWD || MODE == REV) {
            h = max(h, max(e, f));
            if (MODE == FWD) {
                h = max(h, 0);
                const bool gt = h > T.sb;
                T.sb = gt ? h : T.sb;
                T.sp = gt ? cpos + r : T.sp;
            } else {
                T.sp = min(T.sp, h >= T.thr[r] ? cpos + r : 0xffffffffu);
            }
            H[r] = h;
            const int t = h + gap_oe;
            e = max(e + gap_e, t);
            f = max(f + gap_e, t);
        } else {
            // LEFT: the cell took e, or e extends; UP: the cell took f (before e), or f extends
            const int d = h;
            const int m = max(d, f);
            h = max(m, e);
            if (MODE == DIR_SW) h = max(h, 0);
            H[r] = h;
            const int t = h + gap_oe;
            const int e2 = e + gap_e, f2 = f + gap_e;
            const bool left = (e > m) | (e2 > t);
            const bool up = (f > d) | (f2 > t);
            bits |= (left ? 1u : 0u) << (2 * r) | (up ? 2u : 0u) << (2 * r);
            e = max(e2, t);
            f = max(f2, t);
        }
        E[r] = e;
        h = n;
    }
    return bits;
}

// REV: column -1 of reversed row k (query index jj = a_end - k): (-1, -1 + R)
// where the reference re-initialised its arrays (jj <= b_end), else what the
// forward pass left in them.
__device__ __forceinline__ int2 rev_start(const AlignArgs& a, const AlignGroup& G, const AlignLane& L,
                                          const uint32_t lane, const uint32_t k) {
    int2 v = make_int2(-1, -1 + a.gap_extend);
    if (L.used && k <= L.a_end && L.a_end - k > L.b_end)
        v = a.fin[((size_t)G.q_row * 4 + (L.a_end - k)) * 64 + lane];
    return v;
}

template <int MODE>
__global__ void __launch_bounds__(64) sweep_kernel(const AlignArgs a) {
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
    const int Q = a.gap_open, Ge = a.gap_extend, goe = Q + Ge;
    uint2 len = make_uint2(0, 0);
    AlignLane L = {};
    if (MODE == FWD || MODE == DIR_NW) len = a.lens[li];
    if (MODE == REV) L = a.lanes[li];
    // DIR_NW: the lane's last cell (an unused lane, qlen 0, never matches a strip)
    const uint32_t last_strip = (len.x - 1) / R, last_row = (len.x - 1) % R;
    int best = 0, cap = 0;
    uint32_t pos = kAlignNoPos;
    if (MODE == REV) pos = 0xffffffffu;
    const uint32_t* tp = a.tres + ((size_t)G.t_row * 64 + lane);
    int2* bp = a.bnd + ((size_t)G.b_row * 64 + lane);
    const uint32_t ncb = G.nstrips ? G.ncb : 0;

    for (uint32_t s = 0; s < G.nstrips && ncb; s++) {
        strip_profile(prof, mt, a.qres + (((size_t)G.q_row + 2 * s) * 64 + lane), lane);
        // ---- column -1 of the strip
        int H[R], E[R];
        Track T;
        T.sb = 0;
        T.sp = MODE == REV ? pos : kAlignNoPos;
#pragma unroll
        for (int r = 0; r < R; r++) {
            const int i = (int)(s * R) + r;
            if (MODE == FWD) {
                H[r] = 0;
                E[r] = goe;
            } else if (MODE == REV) {
                const int2 v = rev_start(a, G, L, lane, (uint32_t)i);
                H[r] = v.x;
                E[r] = v.y;
                T.thr[r] = (L.used && (uint32_t)i <= L.a_end) ? L.best : 0x7fffffff;
            } else if (MODE == DIR_SW) {
                H[r] = 0;
                E[r] = 0;
            } else {
                H[r] = Q + (i + 1) * Ge;
                E[r] = 2 * Q + (i + 2) * Ge;
            }
        }
        const bool first = s == 0, last = s + 1 == G.nstrips;
        // H(row0 - 1, -1): the diagonal of column 0's top cell
        int hd = 0;
        if (MODE == REV && !first) hd = rev_start(a, G, L, lane, s * R - 1).x;
        if (MODE == DIR_NW && !first) hd = Q + (int)(s * R) * Ge;
        // the first strip's top boundary by formula: H(-1, j) and the F entering row 0
        int top_h = MODE == REV ? -1 : MODE == DIR_NW ? Q + Ge : 0;
        int top_f = MODE == FWD ? goe : MODE == REV ? -1 + Ge : MODE == DIR_NW ? 2 * Q + 2 * Ge : 0;
        const uint32_t fincol = MODE == FWD ? len.y - 1 : 0xffffffffu;
        uint32_t sel[R];   // DIR_NW: all ones for the lane's last row in its last strip
#pragma unroll
        for (int r = 0; r < R; r++)
            sel[r] = (MODE == DIR_NW && s == last_strip && last_row == (uint32_t)r) ? 0xffffffffu : 0u;
        const uint32_t capcol = (MODE == DIR_NW && s == last_strip) ? len.y - 1 : 0xffffffffu;

        uint32_t w_next = tp[0];
        int2 b_next[4];
#pragma unroll
        for (int k = 0; k < 4; k++) b_next[k] = bp[(size_t)k * 64];
        for (uint32_t cb = 0; cb < ncb; cb++) {
            const uint32_t w = w_next;
            int2 b[4];
#pragma unroll
            for (int k = 0; k < 4; k++) b[k] = b_next[k];
            // the next block's residues and boundary, in flight during this block's cells
            const uint32_t nb = cb + 1 < ncb ? cb + 1 : cb;
            w_next = tp[(size_t)nb * 64];
#pragma unroll
            for (int k = 0; k < 4; k++) b_next[k] = bp[((size_t)nb * 4 + k) * 64];
            uint2 pv[4];
#pragma unroll
            for (int k = 0; k < 4; k++) pv[k] = prof[((w >> (8 * k)) & 0xff) * 64 + lane];
            uint32_t dbits[4];
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const uint32_t col = cb * 4 + k;
                const int th = first ? top_h : b[k].x;
                int f = first ? top_f : b[k].y;
                uint32_t cpos = col << 16 | (s * R);
                if (MODE == REV) cpos = (L.used && col <= L.b_end) ? cpos : 0xffff0000u;
                dbits[k] = column<MODE>(pv[k], hd, f, H, E, T, cpos, goe, Ge);
                hd = th;
                if (MODE == DIR_NW) {
                    top_h += Ge;
                    top_f += Ge;
                }
                if (MODE == FWD && col == fincol) {
                    // the lane's own last column: what the reference's arrays hold after its forward pass
                    int2* fp = a.fin + (((size_t)G.q_row * 4 + (size_t)s * R) * 64 + lane);
#pragma unroll
                    for (int r = 0; r < R; r++) fp[(size_t)r * 64] = make_int2(H[r], E[r]);
                }
                if (MODE == DIR_NW) {
                    // NW's score: H of the lane's own last row at its last column (selected by mask, as
                    // pairs_kernel does: a predicated block here costs the kernel its registers)
                    uint32_t hs = 0;
#pragma unroll
                    for (int r = 0; r < R; r++) hs |= (uint32_t)H[r] & sel[r];
                    cap = col == capcol ? (int)hs : cap;
                }
                b[k] = make_int2(H[R - 1], f);
            }
            if (MODE == DIR_SW || MODE == DIR_NW)
                a.dir[((size_t)G.d_row + (size_t)s * ncb + cb) * 64 + lane] =
                    make_uint2(dbits[0] | dbits[1] << 16, dbits[2] | dbits[3] << 16);
            if (!last) {
#pragma unroll
                for (int k = 0; k < 4; k++) bp[((size_t)cb * 4 + k) * 64] = b[k];
            }
        }
        if (MODE == FWD) {
            // strips are not the reference's order: the smaller column wins, then the earlier strip
            // (col << 16 | row compares exactly so)
            const bool take = T.sb > best || (T.sb == best && T.sp < pos);
            best = take ? T.sb : best;
            pos = take ? T.sp : pos;
        }
        if (MODE == REV) pos = T.sp;
    }
    if (MODE == FWD) a.out[li] = make_int2(best, (int)pos);
    if (MODE == REV) a.out[li] = make_int2((int)pos, 0);
    if (MODE == DIR_NW) a.out[li] = make_int2(cap, 0);
}

// The reference's cigar() walk (align.cpp), one lane per pair: from the end
// cell while both indices are inside the region; LEFT steps along the target
// ('I'), else UP along the query ('D'), else diagonal ('M').  Each step is one
// dependent 2-byte load of the lane's own direction bits.
__global__ void __launch_bounds__(64) walk_kernel(const AlignArgs a) {
    const uint32_t lane = threadIdx.x;
    const uint32_t g = blockIdx.x;
    const AlignGroup G = a.groups[g];
    const size_t li = (size_t)g * 64 + lane;
    const AlignLane L = a.lanes[li];
    uint32_t n = 0;
    if (L.used && L.cap) {
        const uint16_t* dp = (const uint16_t*)a.dir;
        uint32_t* rp = a.runs + L.slot;
        int i = (int)L.a_end, j = (int)L.b_end;
        const int ib = (int)L.a_begin, jb = (int)L.b_begin;
        uint32_t op = 3, cnt = 0;
        while (i >= ib && j >= jb) {
            const size_t row = (size_t)G.d_row + (size_t)((uint32_t)i / R) * G.ncb + (uint32_t)j / 4;
            const uint32_t d = (dp[(row * 64 + lane) * 4 + ((uint32_t)j & 3)] >> (2 * ((uint32_t)i % R))) & 3u;
            const uint32_t o = (d & 1) ? kOpI : (d & 2) ? kOpD : kOpM;
            if (o == op) {
                cnt++;
            } else {
                if (cnt && n < L.cap) rp[n++] = cnt << 2 | op;
                op = o;
                cnt = 1;
            }
            j -= o != kOpD;
            i -= o != kOpI;
        }
        if (cnt && n < L.cap) rp[n++] = cnt << 2 | op;
    }
    a.out[li] = make_int2((int)n, 0);
}

}  // namespace

hipError_t launch_pairs_align(int pass, bool nw, const AlignArgs& a, hipStream_t st) {
    if (a.ngroups == 0) return hipSuccess;
    const void* k = pass == 0   ? (const void*)&sweep_kernel<FWD>
                    : pass == 1 ? (const void*)&sweep_kernel<REV>
                    : pass == 2 ? (nw ? (const void*)&sweep_kernel<DIR_NW> : (const void*)&sweep_kernel<DIR_SW>)
                                : (const void*)&walk_kernel;
    (void)ssa_launch(k, dim3(a.ngroups), dim3(64), 0, st, a);
    return hipGetLastError();
}

}  // namespace ssa
