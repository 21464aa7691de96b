// promote_wave.h -- the pair kernel's wave-level exact SW scorer (DESIGN.md
// §3.1, fourth round): one wave scores one DB entry against the whole query,
// score only, int32, affine gaps.  The geometry is align_wave.hip's forward
// sweep at one pass: lane l holds RL consecutive query rows from row l * RL, H
// and E of them in VGPRs, and the entry's columns sweep through the lanes as a
// skewed wavefront -- at step t lane l computes column t - l of its rows; H and
// F of the row above and the column's residue arrive by DPP wave_shr:1.  Lane
// 0's residues are fetched 64 columns at a time, one column per lane, a block
// ahead, and picked per step with v_readlane.
//
// The profile lives in the workgroup's LDS, shared by its waves:
// prof[code][row] as int16, 64 * RL rows per code (rows past the query: 0), so
// a lane reads its RL rows' scores against one code with one ds_read.  Rows
// past the query need no mask: their profile is 0, so such a cell's H is at
// most that of a real cell above it or to its left.
#pragma once
#include "kernels.h"

namespace ssa {

typedef uint32_t promo_u32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) const promo_u32x4 promo_lds_u4;

__device__ __forceinline__ int32_t promo_shr1(int32_t lane0_value, int32_t v) {
    // DPP wave_shr:1 -- lane l receives lane l-1's v, lane 0 keeps lane0_value
    return __builtin_amdgcn_update_dpp(lane0_value, v, 0x138, 0xf, 0xf, false);
}

// The workgroup writes the profile of query[0 .. m) under `matrix` (compact or
// class code x query code, TableArgs::matrix) for codes [0, alpha) to the LDS
// at dword kPromoteProf.  The caller's barrier follows.
__device__ __forceinline__ void promote_profile(uint32_t* lds, const uint8_t* query, const int64_t* matrix, uint32_t m,
                                                uint32_t alpha, uint32_t tid, uint32_t nthreads) {
    int16_t* const prof = (int16_t*)(lds + kPromoteProf);
    constexpr uint32_t ROWS = 64 * kPromoteRL;
    for (uint32_t row = tid; row < ROWS; row += nthreads) {
        const bool real = row < m;
        const uint32_t qc = real ? (uint32_t)query[row] & 31u : 0u;
#pragma unroll 4
        for (uint32_t c = 0; c < alpha; c++) prof[c * ROWS + row] = real ? (int16_t)matrix[(c << 5) + qc] : (int16_t)0;
    }
}

// The SW score of the entry whose residue bytes start at rb (the lane-blocked
// layout: column c at byte (c >> 4) * 1024 + (c & 15)) and run ncols columns,
// against the profile in LDS.  lmax: the last lane that holds a query row.
// Every lane of the wave calls it with the same arguments; every loop is
// bounded by ncols.
__device__ __forceinline__ uint32_t promote_score(const uint8_t* rb, uint32_t ncols, uint32_t lmax, uint32_t alpha,
                                                  int goe, int ge, uint32_t lane) {
    constexpr int RL = kPromoteRL;
    static_assert(RL == 8, "one 16-byte profile read per step");
    auto dcode = [&](uint32_t col) -> uint32_t {
        return col < ncols ? min((uint32_t)rb[(size_t)(col >> 4) * 1024 + (col & 15)], alpha - 1) : 0u;
    };
    auto slice = [&](uint32_t code) -> promo_u32x4 {
        return *(promo_lds_u4*)(uintptr_t)(kPromoteProf * 4 + code * (64 * RL * 2) + lane * (RL * 2));
    };
    int H[RL], E[RL];
#pragma unroll
    for (int r = 0; r < RL; r++) {
        H[r] = 0;
        E[r] = goe;
    }
    const bool lact = lane <= lmax;
    int hdiag = 0, hbot = 0, fbot = 0, sb = 0;
    uint32_t cb_cur = dcode(1 + lane), cb_nxt = 0;
    // the residues run one step ahead of the DP: at step t lane l receives
    // column t + 1 - l and issues the LDS load of its profile slice
    uint32_t code = (uint32_t)promo_shr1((int)dcode(0), 0);
    promo_u32x4 pv_next = slice(code);
    const uint32_t steps = ncols + lmax;
#pragma unroll 1
    for (uint32_t ub = 0; ub < steps; ub += 64) {
        if (ub > 0) cb_cur = cb_nxt;
        cb_nxt = dcode(ub + 65 + lane);
        const uint32_t tend = min(ub + 64, steps);
#pragma unroll 1
        for (uint32_t t = ub; t < tend; t++) {
            const promo_u32x4 pv = pv_next;
            code = (uint32_t)promo_shr1(__builtin_amdgcn_readlane((int)cb_cur, (int)(t - ub)), (int)code);
            pv_next = slice(code);
            const int hu = promo_shr1(0, hbot);
            int f = promo_shr1(goe, fbot);
            const int j = (int)t - (int)lane;
            if (lact && j >= 0 && j < (int)ncols) {
                const uint32_t w[4] = {pv.x, pv.y, pv.z, pv.w};
                int h = hdiag;
#pragma unroll
                for (int r = 0; r < RL; r++) {
                    const int n = H[r];
                    h += (int)(int16_t)(w[r >> 1] >> (16 * (r & 1)));
                    h = max(max(h, 0), max(E[r], f));
                    sb = max(sb, h);
                    H[r] = h;
                    const int tt = h + goe;
                    E[r] = max(E[r] + ge, tt);
                    f = max(f + ge, tt);
                    h = n;
                }
                hdiag = hu;
                hbot = H[RL - 1];
                fbot = f;
            }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sb = max(sb, __shfl_xor(sb, o));
    return (uint32_t)__builtin_amdgcn_readfirstlane(sb);
}

}  // namespace ssa
