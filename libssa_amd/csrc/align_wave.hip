// align_wave.hip -- the wave aligner's kernels (layout: align_wave.h; host
// side: align_wave.cpp).  The geometry is long_kernel's
// (kernels.hip) at one wave per entry: lane l holds RL consecutive query rows
// of the current pass, H and E of them in VGPRs, and the pair's columns sweep
// through the lanes as a skewed wavefront -- at step t lane l computes column
// t - l of its rows.  H and F of the row above (lane l - 1's last row at that
// column, made one step earlier) and the column's residue arrive by DPP
// wave_shr:1; lane 0 takes them from the top boundary (first pass) or from the
// previous pass's bottom row, which lane 63 left in the pair's scratch row.
// Lane 0's inputs are fetched 64 columns at a time, one column per lane, a
// block ahead, and picked per step with v_readlane; the steps run in rounds of
// 64, and only between two rounds does the wave wait for a load.  Each wave builds the
// pass's profile in LDS: prof[code][lane] = the scores of the lane's RL rows
// against that code, read with one ds_read per step.
//
// wave_sweep<MODE, RL> is that sweep with what the reference's traceback
// (align.cpp) needs of it; the semantics of the four modes are pairs_align.hip's
// (its header and DESIGN.md §9.1), cell for cell:
//   FWD     SW forward: the maximum and the first cell that holds it in the
//           reference's order (target index outer, query index inner), and
//           every row's (H, E) after the pair's last column (fin)
//   REV     SW reverse from the end cell by index arithmetic, no floor: the
//           first cell that reaches the maximum
//   DIR_SW / DIR_NW   two direction bits per cell (and NW's score)
// wave_walk then follows the bits from the end cell, one lane per pair.
// Between the passes nothing goes to the host: each reads the pair's record
// (WaveRec) the pass before wrote.
//
// One wave per pair and nothing shared between waves: no flag, no ring, no
// wait on another wave.  Every loop is bounded by the pair's lengths.
//
// FWD needs no mask on rows past the query (their profile is 0; columns past
// the target are never swept): pairs_align.hip's argument holds as written --
// such a cell's H is at most that of a real cell above it or to its left,
// which comes earlier in (column, row) order, and a lane keeps a candidate
// only when it is greater in sweep order (column outer, row inner for the
// lane's own rows), lanes and passes merge by (greater value, then smaller
// col << 16 | row).
#include "align_wave.h"
#include "launch.h"

namespace ssa {
namespace {

enum Mode { FWD = 0, REV = 1, DIR_SW = 2, DIR_NW = 3 };

constexpr uint32_t kOpM = 0, kOpI = 1, kOpD = 2;

__device__ __forceinline__ int32_t shr1(int32_t lane0_value, int32_t v) {
    // DPP wave_shr:1 -- lane l receives lane l-1's v, lane 0 keeps lane0_value
    return __builtin_amdgcn_update_dpp(lane0_value, v, 0x138, 0xf, 0xf, false);
}

// profile bytes per (code, lane): RL scores in 4, 8 or 16 bytes (one ds_read)
constexpr int rl_pad(int rl) { return rl <= 4 ? 4 : rl <= 8 ? 8 : 16; }

template <int N>
struct alignas(N * 4) Slice {
    uint32_t v[N];
};

template <int BYTES> struct DirElem { using type = uint8_t; };
template <> struct DirElem<2> { using type = uint16_t; };
template <> struct DirElem<4> { using type = uint32_t; };

// REV: column -1 of reversed row k (query index jj = a_end - k): (-1, -1 + R)
// where the reference re-initialised its arrays (jj <= b_end), else what the
// forward pass left in them.
__device__ __forceinline__ int2 rev_start(const int2* fin, const uint32_t a_end, const uint32_t b_end, const int ge,
                                          const uint32_t k) {
    int2 v = make_int2(-1, -1 + ge);
    if (k <= a_end && a_end - k > b_end) v = fin[a_end - k];
    return v;
}

template <int MODE, int RL>
__global__ void __launch_bounds__(64) wave_sweep(const WaveArgs a) {
    constexpr int RLP = rl_pad(RL);
    constexpr uint32_t RP = 64 * RL;                  // rows per pass
    using Elem = typename DirElem<wave_dir_elem(RL)>::type;
    __shared__ __attribute__((aligned(16))) uint8_t prof[32 * 64 * RLP];   // [code][lane][RLP]
    __shared__ uint32_t mt[32 * 8];                                         // mt[q][d], a row = 8 dwords
    const uint32_t lane = threadIdx.x;
    for (uint32_t i = lane; i < 32 * 8; i += 64) mt[i] = ((const uint32_t*)a.mt)[i];
    __syncthreads();
    const WavePair P = a.pairs[blockIdx.x];
    WaveRec* rec = a.rec + blockIdx.x;
    // ---- the extents of this pass and what the passes before found
    uint32_t nrows = P.qlen, ncols = P.dlen, a_end = 0, b_end = 0;
    int best = 0;
    if (MODE == REV || MODE == DIR_SW) {
        if (rec->state != kWaveOk) return;
        a_end = rec->a_end;
        b_end = rec->b_end;
        best = rec->score;
        if (a_end >= P.qlen || b_end >= P.dlen) {     // (cannot happen: wave_fwd checks what it writes)
            if (lane == 0) rec->state = kWaveNoCell;
            return;
        }
        nrows = a_end + 1;
        ncols = b_end + 1;
    }
    const uint8_t* qs = a.codes + P.q_off;
    const uint8_t* ds = a.codes + P.d_off;
    const int2* fin = a.fin + P.fin_off;
    const int Q = a.gap_open, Ge = a.gap_extend, goe = Q + Ge;
    const uint32_t npass = (nrows + RP - 1) / RP;
    const uint32_t T = ncols + 63;                    // steps of a pass in dir
    Elem* dirp = (Elem*)(a.dir + P.dir_off);
    int tb = 0;                                       // FWD: the maximum
    uint32_t tp = MODE == REV ? 0xffffffffu : kWaveNoPos;
    int H[RL], E[RL];

    for (uint32_t p = 0; p < npass; p++) {
        const uint32_t i0 = p * RP + lane * RL;       // the lane's first row
        const uint32_t lmax = (min(nrows - p * RP, RP) - 1) / RL;   // last lane holding rows
        const bool lact = lane <= lmax;
        const bool lastp = p + 1 == npass;
        // ---- the pass's profile (rows past the extent: 0); the fence orders the
        // previous pass's scratch stores before this pass's loads of them
        __threadfence();
        __syncthreads();
#pragma unroll 1
        for (int r = 0; r < RLP; r++) {
            const uint32_t i = i0 + (uint32_t)r;
            const bool real = r < RL && i < nrows;
            const uint32_t qc = real ? (uint32_t)qs[MODE == REV ? a_end - i : i] & 31u : 0u;
#pragma unroll
            for (int cw = 0; cw < 8; cw++) {
                const uint32_t w = real ? mt[qc * 8 + cw] : 0u;
#pragma unroll
                for (int b = 0; b < 4; b++)
                    prof[(size_t)(((cw * 4 + b) * 64 + lane) * RLP + r)] = (uint8_t)(w >> (8 * b));
            }
        }
        __syncthreads();
        // ---- column -1 of the lane's rows, and H(i0 - 1, -1)
        int thr[RL];                                  // REV: the score to reach, INT_MAX outside the rectangle
#pragma unroll
        for (int r = 0; r < RL; r++) {
            const int i = (int)i0 + r;
            thr[r] = 0x7fffffff;
            if (MODE == FWD) {
                H[r] = 0;
                E[r] = goe;
            } else if (MODE == REV) {
                const int2 v = rev_start(fin, a_end, b_end, Ge, (uint32_t)i);
                H[r] = v.x;
                E[r] = v.y;
                if ((uint32_t)i <= a_end) thr[r] = best;
            } else if (MODE == DIR_SW) {
                H[r] = 0;
                E[r] = 0;
            } else {
                H[r] = Q + (i + 1) * Ge;
                E[r] = 2 * Q + (i + 2) * Ge;
            }
        }
        int hdiag = 0;
        if (MODE == REV && i0 > 0) hdiag = rev_start(fin, a_end, b_end, Ge, i0 - 1).x;
        if (MODE == DIR_NW && i0 > 0) hdiag = Q + (int)i0 * Ge;
        int sb = 0;                                   // FWD: the pass's maximum of this lane
        uint32_t sp = MODE == REV ? tp : kWaveNoPos;
        // ---- lane 0's inputs: column 0 by itself, then 64 columns per block, a block ahead (lane k of
        // block b holds column 64 b + 1 + k); the blocks change between two rounds of 64 steps, so no
        // step waits for memory
        int64_t* swr = a.scr + P.scr_off + (size_t)(p & 1) * P.dlen;
        const int64_t* srd = a.scr + P.scr_off + (size_t)((p & 1) ^ 1) * P.dlen;
        auto dcode = [&](uint32_t col) -> uint32_t {
            return col < ncols ? (uint32_t)ds[MODE == REV ? b_end - col : col] : 0u;   // (masked at its use)
        };
        auto srow = [&](uint32_t col) -> int64_t {
            return (p > 0 && col < ncols) ? __hip_atomic_load(srd + col, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
                                          : (int64_t)0;
        };
        uint32_t cb_cur = dcode(1 + lane), cb_nxt = 0;
        int64_t sb_cur = srow(1 + lane), sb_nxt = 0;
        // the residues (and a later pass's row above) run one step ahead of the DP: at step t lane l
        // receives column t + 1 - l and issues the LDS load of its profile slice, used at step t + 1
        // (the load's latency off the step's dependency chain, as long_kernel)
        uint32_t code = (uint32_t)shr1((int)(dcode(0) & 31u), 0);
        Slice<RLP / 4> pv_next = *(const Slice<RLP / 4>*)(prof + (size_t)((code * 64 + lane) * RLP));
        int h0n, f0n;
        {
            const int64_t v = srow(0);
            h0n = (int)(uint32_t)v;
            f0n = (int)(v >> 32);
        }
        int hbot = 0, fbot = 0;
        const uint32_t steps = ncols + lmax;          // the last lane's last column
#pragma unroll 1
        for (uint32_t ub = 0; ub < steps; ub += 64) {
        if (ub > 0) {
            cb_cur = cb_nxt;
            sb_cur = sb_nxt;
        }
        cb_nxt = dcode(ub + 65 + lane);
        sb_nxt = srow(ub + 65 + lane);
        const uint32_t tend = min(ub + 64, steps);
#pragma unroll 1
        for (uint32_t t = ub; t < tend; t++) {
            const uint32_t tl = t - ub;
            const Slice<RLP / 4> pv = pv_next;
            code = (uint32_t)shr1(__builtin_amdgcn_readlane((int)cb_cur, (int)tl) & 31, (int)code);
            pv_next = *(const Slice<RLP / 4>*)(prof + (size_t)((code * 64 + lane) * RLP));
            // the column entering lane 0 at this step: H(i0 - 1, t) and the F entering row i0
            int h0, f0;
            if (p == 0) {
                h0 = MODE == REV ? -1 : MODE == DIR_NW ? Q + ((int)t + 1) * Ge : 0;
                f0 = MODE == FWD ? goe : MODE == REV ? -1 + Ge : MODE == DIR_NW ? 2 * Q + ((int)t + 2) * Ge : 0;
            } else {
                h0 = h0n;
                f0 = f0n;
                h0n = __builtin_amdgcn_readlane((int)(uint32_t)sb_cur, (int)tl);
                f0n = __builtin_amdgcn_readlane((int)(sb_cur >> 32), (int)tl);
            }
            const int hu = shr1(h0, hbot);
            int f = shr1(f0, fbot);
            const int j = (int)t - (int)lane;
            const bool act = lact && j >= 0 && j < (int)ncols;
            uint32_t bits = 0;
            if (act) {
                const uint32_t cpos = (uint32_t)j << 16 | i0;
                int h = hdiag;
#pragma unroll
                for (int r = 0; r < RL; r++) {
                    const int n = H[r];
                    int e = E[r];
                    h += (int)(int8_t)(pv.v[r >> 2] >> (8 * (r & 3)));
                    if (MODE == FWD || MODE == REV) {
                        h = max(h, max(e, f));
                        if (MODE == FWD) {
                            h = max(h, 0);
                            const bool gt = h > sb;
                            sb = gt ? h : sb;
                            sp = gt ? cpos + r : sp;
                        } else {
                            sp = min(sp, h >= thr[r] ? cpos + r : 0xffffffffu);
                        }
                        H[r] = h;
                        const int tt = h + goe;
                        e = max(e + Ge, tt);
                        f = max(f + Ge, tt);
                    } else {
                        // LEFT: the cell took e, or e extends; UP: the cell took f (before e), or f extends
                        const int d = h;
                        const int m = max(d, f);
                        h = max(m, e);
                        if (MODE == DIR_SW) h = max(h, 0);
                        H[r] = h;
                        const int tt = h + goe;
                        const int e2 = e + Ge, f2 = f + Ge;
                        // (as sign bits, not compares: 2 RL compare results per step do not fit the
                        // scalar registers; every difference stays far inside int32 under the host's bound)
                        const uint32_t left = ((uint32_t)(m - e) | (uint32_t)(tt - e2)) >> 31;
                        const uint32_t up = ((uint32_t)(d - f) | (uint32_t)(tt - f2)) >> 31;
                        bits |= left << (2 * r) | up << (2 * r + 1);
                        e = max(e2, tt);
                        f = max(f2, tt);
                    }
                    E[r] = e;
                    h = n;
                }
                hdiag = hu;
                hbot = H[RL - 1];
                fbot = f;
                if (MODE == FWD && j == (int)ncols - 1) {
                    // the pair's last column: what the reference's arrays hold after its forward pass
                    int2* fp = a.fin + P.fin_off;
#pragma unroll
                    for (int r = 0; r < RL; r++)
                        if (i0 + r < nrows) fp[i0 + r] = make_int2(H[r], E[r]);
                }
                if (!lastp && lane == 63)
                    __hip_atomic_store(swr + j, (int64_t)(uint32_t)hbot | ((int64_t)fbot << 32), __ATOMIC_RELAXED,
                                       __HIP_MEMORY_SCOPE_AGENT);
            }
            if (MODE == DIR_SW || MODE == DIR_NW) dirp[((size_t)p * T + t) * 64 + lane] = (Elem)bits;
        }
        }
        if (MODE == FWD) {
            // passes are not the reference's order: the smaller column wins, then the earlier row
            const bool take = sb > tb || (sb == tb && sp < tp);
            tb = take ? sb : tb;
            tp = take ? sp : tp;
        }
        if (MODE == REV) tp = sp;
    }

    // ---- the record
    if (MODE == FWD) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const int ob = __shfl_xor(tb, off);
            const uint32_t op = (uint32_t)__shfl_xor((int)tp, off);
            const bool take = ob > tb || (ob == tb && op < tp);
            tb = take ? ob : tb;
            tp = take ? op : tp;
        }
        if (lane == 0) {
            WaveRec R = {};
            R.score = tb;
            R.state = kWaveZero;
            if (tb > 0) {
                R.state = kWaveNoCell;
                if (tp < kWaveNoPos && (tp & 0xffff) < P.qlen && (tp >> 16) < P.dlen) {
                    R.a_end = tp & 0xffff;
                    R.b_end = tp >> 16;
                    R.state = kWaveOk;
                }
            }
            *rec = R;
        }
    }
    if (MODE == REV) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) tp = min(tp, (uint32_t)__shfl_xor((int)tp, off));
        if (lane == 0) {
            if (tp >= kWaveNoPos || (tp & 0xffff) > a_end || (tp >> 16) > b_end) {
                rec->state = kWaveNoCell;
            } else {
                rec->a_begin = a_end - (tp & 0xffff);
                rec->b_begin = b_end - (tp >> 16);
            }
        }
    }
    if (MODE == DIR_NW) {
        // NW's score: H of the last row at the last column (the lanes keep their last column's H)
        const uint32_t il = (P.qlen - 1) % RP;
        int hs = 0;
#pragma unroll
        for (int r = 0; r < RL; r++) hs = (il % RL == (uint32_t)r) ? H[r] : hs;
        if (lane == il / RL) {
            WaveRec R = {};
            R.score = hs;
            R.a_end = P.qlen - 1;
            R.b_end = P.dlen - 1;
            R.state = kWaveOk;
            *rec = R;
        }
    }
}

// The reference's cigar() walk (align.cpp), one lane per pair: from the end
// cell while both indices are inside the region; LEFT steps along the target
// ('I'), else UP along the query ('D'), else diagonal ('M').  Each step is one
// dependent load of the cell's lane element; it moves one index down, so the
// loop ends within (rows + columns of the region) steps.
__global__ void __launch_bounds__(64) wave_walk(const WaveArgs a) {
    const uint32_t pi = blockIdx.x * 64 + threadIdx.x;
    if (pi >= a.npairs) return;
    const WavePair P = a.pairs[pi];
    WaveRec* rec = a.rec + pi;
    if (rec->state != kWaveOk) return;
    const uint32_t a_end = rec->a_end, b_end = rec->b_end;
    int i = (int)a_end, j = (int)b_end;
    const int ib = (int)rec->a_begin, jb = (int)rec->b_begin;
    if (a_end >= P.qlen || b_end >= P.dlen || ib > i || jb > j) {
        rec->state = kWaveNoCell;
        return;
    }
    const uint32_t rl = a.rl, rp = 64 * rl, eb = wave_dir_elem(rl);
    const size_t T = (size_t)b_end + 1 + 63;
    const uint8_t* dp = a.dir + P.dir_off;
    uint32_t* rp_out = a.runs + P.runs_off;
    const uint32_t cap = P.qlen + P.dlen;
    uint32_t n = 0, op = 3, cnt = 0;
    // cell (i, j): pass pp, lane li, row r of the lane -- kept as i moves up, no division per step
    uint32_t pp = (uint32_t)i / rp, li = ((uint32_t)i % rp) / rl, r = (uint32_t)i % rl;
    while (i >= ib && j >= jb) {
        const size_t idx = (((size_t)pp * T + (uint32_t)j + li) * 64 + li) * eb;
        const uint32_t w = eb == 1 ? (uint32_t)dp[idx] : eb == 2 ? (uint32_t) * (const uint16_t*)(dp + idx)
                                                                 : *(const uint32_t*)(dp + idx);
        const uint32_t d = (w >> (2 * r)) & 3u;
        const uint32_t o = (d & 1) ? kOpI : (d & 2) ? kOpD : kOpM;
        if (o == op) {
            cnt++;
        } else {
            if (cnt && n < cap) rp_out[n++] = cnt << 2 | op;
            op = o;
            cnt = 1;
        }
        j -= o != kOpD;
        if (o != kOpI) {
            i--;
            if (r > 0) {
                r--;
            } else {
                r = rl - 1;
                if (li > 0) {
                    li--;
                } else {
                    li = 63;
                    pp--;               // (wraps only when i has left the region: the loop ends)
                }
            }
        }
    }
    if (cnt && n < cap) rp_out[n++] = cnt << 2 | op;
    rec->nruns = n;
}

template <int MODE>
const void* sweep_of(uint32_t rl) {
    switch (rl) {
#define WAVE_RL(N) case N: return (const void*)&wave_sweep<MODE, N>;
        WAVE_RL(1) WAVE_RL(2) WAVE_RL(3) WAVE_RL(4) WAVE_RL(5) WAVE_RL(6) WAVE_RL(7) WAVE_RL(8)
        WAVE_RL(9) WAVE_RL(10) WAVE_RL(12) WAVE_RL(16)
#undef WAVE_RL
    }
    return nullptr;
}

}  // namespace

hipError_t launch_align_wave(int pass, bool nw, const WaveArgs& a, hipStream_t st) {
    if (a.npairs == 0) return hipSuccess;
    if (pass == 3) {
        (void)ssa_launch((const void*)&wave_walk, dim3((a.npairs + 63) / 64), dim3(64), 0, st, a);
        return hipGetLastError();
    }
    const void* k = pass == 0   ? sweep_of<FWD>(a.rl)
                    : pass == 1 ? sweep_of<REV>(a.rl)
                                : (nw ? sweep_of<DIR_NW>(a.rl) : sweep_of<DIR_SW>(a.rl));
    if (!k) return hipErrorInvalidValue;
    (void)ssa_launch(k, dim3(a.npairs), dim3(64), 0, st, a);
    return hipGetLastError();
}

}  // namespace ssa
