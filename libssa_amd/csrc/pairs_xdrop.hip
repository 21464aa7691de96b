// pairs_xdrop.hip -- the X-drop end pass (layout: pairs_xdrop.h; host side:
// pairs_xdrop.cpp).  xdrop_kernel is
// local_kernel<false, false, true>'s sweep (pairs_local.hip: one pair per
// lane, query rows in strips of 8 held in VGPRs, the swept column blocks of
// the strip's BandStrip, cells outside the lane's band masked to kBandNegInf
// by index, the bnd row buffer between strips) -- no cell is pruned, so every
// H, E and F is that pass's.  What changes is which cells may end the
// alignment:
//   * inside a strip the lane keeps, per ROW, the greatest finite H and the
//     column that first reached it (strictly greater: columns ascend in a
//     strip).  A row's slot starts at kEmpty, the level below which a value is
//     minus infinity's, so a row without a finite cell stays there: an empty
//     row is tested, never subtracted.  Candidates are taken BY INDEX: a
//     column past the lane's last is capped to INT_MIN, and a row past its
//     last is never read;
//   * at the end of the strip the lane walks its real rows in ascending order
//     with the rule of the definition: an empty row is passed over; a row
//     whose maximum lies more than xdrop below best is the drop row and the
//     lane is DEAD from there; else a greater maximum, or an equal one in a
//     smaller column than the end cell's, moves the end cell.  best starts at
//     0 with no end cell, so a result of 0 is the empty alignment.
// A dead lane goes on computing -- the wave stays convergent and the bnd rows
// keep their protocol -- but its candidates are ignored.  Before each strip
// the wave leaves the strip loop when every lane is dead or has no real row
// left: one __all, nothing between waves.  The strips it entered are reported
// per group, so that the host counts what was swept.
//
// Arithmetic.  Real values lie inside +-2^29 and kEmpty is -2^29, so best - m
// of a real row stays below 2^30 in int32, and an xdrop of 2^30 (the host
// clamps to it) never stops a lane.  Masking and the bound are
// pairs_local.hip's, unchanged.
#include "launch.h"
#include "pairs_xdrop.h"

namespace ssa {
namespace {

constexpr int R = kPairsRows;
constexpr int NEG = kBandNegInf;
constexpr int kEmpty = NEG / 2;
static_assert(R == 8, "one uint2 per (code, lane) holds the strip's scores");

__device__ __forceinline__ int score_of(const uint2 pv, const int r) {
    return (int)(int8_t)((r < 4 ? pv.x : pv.y) >> (8 * (r & 3)));
}

// the lane's strip profile: prof[code][lane] = M[code][rows s*R .. s*R + R) (as local_kernel)
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

// INT_MAX where 0 <= x <= span, else NEG, in plain arithmetic (pairs_banded.hip says why)
__device__ __forceinline__ int cap_of(const int x, const int span) {
    const int bad = (x | (span - x)) >> 31;
    return (bad & NEG) | (~bad & 0x7fffffff);
}

// INT_MAX where x >= 0, else INT_MIN
__device__ __forceinline__ int keep_of(const int x) { return 0x7fffffff ^ (x >> 31); }

// One column of a strip: local_kernel's score column without the floor.
template <bool MASK>
__device__ __forceinline__ void column(const uint2 pv, int h, int& f, int (&H)[R], int (&E)[R], const int gap_oe,
                                       const int gap_e, const int u, const uint32_t span) {
#pragma unroll
    for (int r = 0; r < R; r++) {
        const int n = H[r];
        int e = E[r];
        h += score_of(pv, r);
        const bool exists = !MASK || (uint32_t)(u - r) <= span;
        h = max(h, max(e, f));
        h = exists ? h : NEG;
        H[r] = h;
        const int t = h + gap_oe;
        e = max(e + gap_e, t);
        f = max(f + gap_e, t);
        E[r] = e;
        h = n;
    }
}

// What a lane keeps of a strip's end candidates: every row's greatest finite H and its smallest column.
struct RowTrack {
    int m[R];
    uint32_t c[R];
};

// What a lane knows of its own shape and band in this strip (as local_kernel).
struct LaneShape {
    uint32_t ccol;    // the lane's last column, dlen - 1
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

// One block of 4 columns (pairs_local.hip's block()).  COLCAP: the block holds columns past the end of a
// lane that still has real rows in the strip; a candidate is capped to INT_MIN there.
template <bool COLCAP, bool MASK>
__device__ __forceinline__ void block(const uint2 (&pv)[4], int2 (&b)[4], const bool first, const uint32_t cb, Edge& X,
                                      const int top_step, int (&H)[R], int (&E)[R], RowTrack& T, const LaneShape& L,
                                      const int goe, const int Ge) {
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
        column<MASK>(pv[k], X.hd, f, H, E, goe, Ge, u, L.span);
        X.hd = th;
        X.top_h += top_step;
        X.top_f += top_step;
        const int ccap = COLCAP ? keep_of((int)L.ccol - (int)col) : 0x7fffffff;
#pragma unroll
        for (int r = 0; r < R; r++) {
            int v = H[r];
            if (COLCAP) v = min(v, ccap);
            const bool take = v > T.m[r];
            T.m[r] = take ? v : T.m[r];
            T.c[r] = take ? col : T.c[r];
        }
        b[k] = make_int2(H[R - 1], f);
    }
}

// The swept blocks [S.cb0, S.cb0 + S.ncb) of one strip (S.ncb >= 1).  col_min: the smallest last column
// among the lanes with real rows in the strip.
__device__ __forceinline__ void sweep(const BandedArgs& a, const BandGroup& G, const BandStrip& S, const uint2* prof,
                                      const uint32_t lane, const uint32_t s, const int in_lo, const int in_hi,
                                      int (&H)[R], int (&E)[R], RowTrack& T, const LaneShape& L,
                                      const uint32_t col_min) {
    const int Q = a.gap_open, Ge = a.gap_extend, goe = Q + Ge;
    const bool fqb = a.ends & kFreeQBegin, fdb = a.ends & kFreeDBegin;
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
    uint32_t w_next = tp[(size_t)cb0 * 64];
    int2 b_next[4];
#pragma unroll
    for (int k = 0; k < 4; k++) b_next[k] = bp[((size_t)cb0 * 4 + k) * 64];
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
        if (__builtin_expect(cb * 4 + 3 > col_min, 0))
            block<true, true>(pv, b, first, cb, X, top_step, H, E, T, L, goe, Ge);
        else if ((int)cb >= in_lo && (int)cb <= in_hi)
            block<false, false>(pv, b, first, cb, X, top_step, H, E, T, L, goe, Ge);
        else
            block<false, true>(pv, b, first, cb, X, top_step, H, E, T, L, goe, Ge);
        if (!last) {
#pragma unroll
            for (int k = 0; k < 4; k++) bp[((size_t)cb * 4 + k) * 64] = b[k];
        }
    }
}

__global__ void __launch_bounds__(64) xdrop_kernel(const XdropArgs xa) {
    __shared__ uint2 prof[kPairsCodes * 64];
    __shared__ uint4 mt[kPairsCodes * 2];
    const BandedArgs& a = xa.b;
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
    const int Q = a.gap_open, Ge = a.gap_extend, goe = Q + Ge;
    const int xdrop = xa.xdrop;
    // column -1: H(i, -1) = hq0 + (i + 1) * hq1, both 0 where the q begin is free
    const bool fqb = a.ends & kFreeQBegin, fdb = a.ends & kFreeDBegin;
    const int hq0 = fqb ? 0 : Q, hq1 = fqb ? 0 : Ge;
    const bool zero = band.x <= 0 && band.y >= 0;
    // the rule's state: best, the end cell (brow 0xffffffff: none; bcol is then 0, below which no column is), dead
    int best = 0;
    uint32_t bcol = 0, brow = 0xffffffffu;
    bool dead = false;
    LaneShape L;
    L.ccol = len.y - 1;
    L.span = (uint32_t)(band.y - band.x);
    L.top_ok = fdb || zero;
    L.left_ok = fqb || zero;
    uint32_t s = 0;
    for (; s < G.nstrips; s++) {
        const int rows = (int)len.x - (int)(s * R);       // rows r < rows of this strip are real
        const bool alive = rows > 0;
        if (__all(dead || !alive)) break;                 // wave-uniform: nothing below can end an alignment
        const BandStrip S = a.strips[G.s_row + s];
        if (S.ncb == 0) continue;       // no lane has a cell of its band in this strip: its rows are empty
        strip_profile(prof, mt, a.qres + (((size_t)G.q_row + 2 * s) * 64 + lane), lane);
        L.base = (int)(s * R) + band.x;
        L.aspan = (s != 0 || L.top_ok) ? (int)L.span : -1;
        int H[R], E[R];
        RowTrack T;
        const bool from_edge = S.cb0 == 0 && L.left_ok;
#pragma unroll
        for (int r = 0; r < R; r++) {
            const int i = (int)(s * R) + r;
            const bool ex = from_edge && (uint32_t)(-1 - r - L.base) <= L.span;
            H[r] = ex ? hq0 + (i + 1) * hq1 : NEG;
            E[r] = H[r] + goe;
            T.m[r] = kEmpty;
            T.c[r] = 0;
        }
        // the blocks [in_lo, in_hi] in which no lane needs a band mask (as local_kernel)
        int in_lo = (L.base + R - 1 + 3) >> 2, in_hi = (L.aspan + L.base - 4) >> 2;
        if (!alive) in_lo = -(1 << 30);
        if (!alive || in_hi + 1 >= (int)((len.y + 3) >> 2)) in_hi = 1 << 30;
        // the lanes with real rows here; their smallest last column
        uint32_t col_min = alive ? L.ccol : 0xffffffffu;
        for (int o = 32; o; o >>= 1) {
            in_lo = max(in_lo, __shfl_xor(in_lo, o));
            in_hi = min(in_hi, __shfl_xor(in_hi, o));
            col_min = min(col_min, (uint32_t)__shfl_xor((int)col_min, o));
        }
        in_lo = __builtin_amdgcn_readfirstlane(in_lo);
        in_hi = __builtin_amdgcn_readfirstlane(in_hi);
        col_min = __builtin_amdgcn_readfirstlane(col_min);
        sweep(a, G, S, prof, lane, s, in_lo, in_hi, H, E, T, L, col_min);
        // the rule over the lane's real rows, ascending
#pragma unroll
        for (int r = 0; r < R; r++) {
            const int m = T.m[r];
            const bool real = !dead & (r < rows) & (m > kEmpty);
            const bool drop = real & (best - m > xdrop);
            const bool take = real & !drop & ((m > best) | ((m == best) & (T.c[r] < bcol)));
            best = take ? m : best;
            bcol = take ? T.c[r] : bcol;
            brow = take ? s * R + r : brow;
            dead |= drop;
        }
    }
    const uint32_t pos = brow == 0xffffffffu ? 0xffffffffu : (bcol << 16 | (brow & 0xffff));
    a.out[li] = make_int2(best, (int)pos);
    xa.dropped[li] = dead ? 1u : 0u;
    if (lane == 0) xa.entered[g] = s;
}

}  // namespace

hipError_t launch_pairs_xdrop(const XdropArgs& a, hipStream_t st) {
    if (a.b.ngroups == 0) return hipSuccess;
    (void)ssa_launch((const void*)&xdrop_kernel, dim3(a.b.ngroups), dim3(64), 0, st, a);
    return hipGetLastError();
}

}  // namespace ssa
