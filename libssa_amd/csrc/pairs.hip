// pairs.hip -- the batch pair scorer: pairs_kernel<NW> scores one group of
// 64 independent (query, target) pairs per wave, one pair per lane, in exact
// int32 (layout: pairs.h; host side: pairs.cpp).
//
// Unlike the search kernels every lane has a query of its own, so there is no
// shared profile.  Each lane keeps a private STRIP PROFILE in LDS instead:
// at the start of a strip it writes, for each of the 33 target codes, the
// R = 8 int8 scores M[code][own query rows] as one 8-byte word at
// (code * 64 + lane) * 8.  A column is then one ds_read_b64 at an address that
// depends on the lane's own residue; lane l always lands on banks 2l, 2l + 1
// of its 32-lane half, so the read is conflict-free whatever the residues are.
//
// Lanes shorter than the group's sweep are masked BY VALUE: rows past a lane's
// query and columns past its target hold the padding code, which scores 0
// against everything.  With gap penalties <= 0 (pairs.cpp sends anything else
// to the host) no padding cell of SW can exceed the maximum over the lane's
// real cells, so the running maximum needs no mask; an NW lane picks H at its
// own (qlen - 1, dlen - 1) when the sweep passes it.
#include "launch.h"
#include "pairs.h"

namespace ssa {
namespace {

constexpr int R = kPairsRows;
static_assert(R == 8, "one uint2 per (code, lane) holds the strip's scores");

__device__ __forceinline__ int score_of(const uint2 pv, const int r) {
    return (int)(int8_t)((r < 4 ? pv.x : pv.y) >> (8 * (r & 3)));
}

// One column of a strip: h enters as the diagonal H(row0 - 1, j - 1), f as the
// F coming down from the strip above; H[r] / E[r] hold column j - 1 on entry
// and column j on exit (the recurrences of the reference's 64-bit kernels).
template <bool NW>
__device__ __forceinline__ void column(const uint2 pv, int h, int& f, int (&H)[R], int (&E)[R], int& smax,
                                       const int gap_oe, const int gap_e) {
#pragma unroll
    for (int r = 0; r < R; r++) {
        const int n = H[r];
        int e = E[r];
        h += score_of(pv, r);
        h = max(h, max(e, f));
        if (!NW) {
            h = max(h, 0);
            smax = max(smax, h);
        }
        H[r] = h;
        const int t = h + gap_oe;
        e = max(e + gap_e, t);
        f = max(f + gap_e, t);
        E[r] = e;
        h = n;
    }
}

// All columns of one strip.  CAP (NW only): some lane's last row lies in this
// strip, so each column also selects H of the lane's own last row (sel[r] is
// all ones for that row of that lane, else 0) and keeps it at the lane's last
// column.
template <bool NW, bool CAP>
__device__ __forceinline__ void sweep(const PairsArgs& a, const PairsGroup& G, const uint2* prof, const uint32_t lane,
                                      const uint32_t s, int (&H)[R], int (&E)[R], int& smax, int& cap,
                                      const uint32_t (&sel)[R], const uint32_t capcol) {
    const int Q = a.gap_open, Ge = a.gap_extend, goe = Q + Ge;
    const bool first = s == 0, last = s + 1 == G.nstrips;
    const uint32_t* tp = a.tres + ((size_t)G.t_row * 64 + lane);
    int2* bp = a.bnd + ((size_t)G.b_row * 64 + lane);
    // H(row0 - 1, -1): the diagonal of column 0's top cell
    int hd = NW ? (first ? 0 : Q + (int)(s * R) * Ge) : 0;
    // the first strip's top boundary by formula: H(-1, j) and the F entering row 0
    int top_h = NW ? Q + Ge : 0, top_f = NW ? 2 * Q + 2 * Ge : 0;
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
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int th = first ? top_h : b[k].x;
            int f = first ? top_f : b[k].y;
            column<NW>(pv[k], hd, f, H, E, smax, goe, Ge);
            hd = th;
            if (NW) {
                top_h += Ge;
                top_f += Ge;
            }
            if (CAP) {
                uint32_t hs = 0;
#pragma unroll
                for (int r = 0; r < R; r++) hs |= (uint32_t)H[r] & sel[r];
                cap = cb * 4 + k == capcol ? (int)hs : cap;
            }
            b[k] = make_int2(H[R - 1], f);
        }
        if (!last) {
#pragma unroll
            for (int k = 0; k < 4; k++) bp[((size_t)cb * 4 + k) * 64] = b[k];
        }
    }
}

template <bool NW>
__global__ void __launch_bounds__(64) pairs_kernel(const PairsArgs a) {
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
    const PairsGroup G = a.groups[g];
    const uint2 len = a.lens[(size_t)g * 64 + lane];
    // the lane's last cell (an unused lane, qlen 0, never matches a strip)
    const uint32_t last_strip = (len.x - 1) / R, last_row = (len.x - 1) % R;
    const int Q = a.gap_open, Ge = a.gap_extend;
    int smax = 0, cap = 0;
    for (uint32_t s = 0; s < G.nstrips; s++) {
        // ---- the lane's strip profile: prof[code][lane] = M[code][rows s*R .. s*R + R)
        const uint32_t* qp = a.qres + (((size_t)G.q_row + 2 * s) * 64 + lane);
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
        // ---- column -1 of the strip
        int H[R], E[R];
#pragma unroll
        for (int r = 0; r < R; r++) {
            const int i = (int)(s * R) + r;
            H[r] = NW ? Q + (i + 1) * Ge : 0;
            E[r] = NW ? 2 * Q + (i + 2) * Ge : 0;
        }
        uint32_t sel[R];
#pragma unroll
        for (int r = 0; r < R; r++) sel[r] = 0;
        if (NW && __any(s == last_strip)) {
#pragma unroll
            for (int r = 0; r < R; r++) sel[r] = (s == last_strip && last_row == (uint32_t)r) ? 0xffffffffu : 0u;
            const uint32_t capcol = s == last_strip ? len.y - 1 : 0xffffffffu;
            sweep<NW, true>(a, G, prof, lane, s, H, E, smax, cap, sel, capcol);
        } else {
            sweep<NW, false>(a, G, prof, lane, s, H, E, smax, cap, sel, 0xffffffffu);
        }
    }
    a.out[(size_t)g * 64 + lane] = NW ? cap : smax;
}

}  // namespace

hipError_t launch_pairs(int algo, const PairsArgs& a, hipStream_t st) {
    if (a.ngroups == 0) return hipSuccess;
    const void* k = algo ? (const void*)&pairs_kernel<true> : (const void*)&pairs_kernel<false>;
    (void)ssa_launch(k, dim3(a.ngroups), dim3(64), 0, st, a);
    return hipGetLastError();
}

}  // namespace ssa
