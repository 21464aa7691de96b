// above.hip -- above_select: every score at or above a fixed threshold, as
// (position, score) pairs for the host (arguments: above.h; host side:
// engine.cpp device_search).
//
// A thread reads kAbovePer consecutive scores with one 16-byte load.  A wave
// counts its forwarded scores with one ballot per slot: the bits below a lane
// (mbcnt), summed over the slots, are what the lanes before it forward, so
// the wave writes in position order.  The four waves of a block combine their
// counts in LDS and the block reserves its output range with ONE atomic on the
// candidate counter -- a low threshold forwards every entry, and one atomic
// per entry would serialise on that word.  No block waits for another: the
// ranges' order is arbitrary, the host sorts.
#include "above.h"
#include "launch.h"

namespace ssa {
namespace {

constexpr uint32_t kWaves = kAboveThreads / 64;

__global__ void __launch_bounds__(kAboveThreads) above_select(const AboveArgs a) {
    __shared__ uint32_t wave_count[kWaves];
    __shared__ uint32_t block_base;
    const uint32_t tid = blockIdx.x * kAboveThreads + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    // the header words filter_select writes (one host read-back for both)
    if (tid < a.nviews) a.counters[3 + tid] = a.ovf_count[(size_t)tid * a.ovf_stride];
    if (tid == 0 && a.status) a.counters[2] = *a.status;

    const uint32_t e0 = tid * kAbovePer;
    int32_t x[kAbovePer];
    if (e0 + kAbovePer <= a.n) {
        const int4 q = *(const int4*)(a.scores + e0);
        x[0] = q.x, x[1] = q.y, x[2] = q.z, x[3] = q.w;
    } else {
#pragma unroll
        for (uint32_t j = 0; j < kAbovePer; j++) x[j] = e0 + j < a.n ? a.scores[e0 + j] : 0;
    }
    bool take[kAbovePer];
    uint32_t before = 0, total = 0;      // forwarded by the lanes below this one / by the wave
#pragma unroll
    for (uint32_t j = 0; j < kAbovePer; j++) {
        take[j] = e0 + j < a.n && (x[j] == INT32_MIN || x[j] >= a.t32);
        const uint64_t b = __ballot(take[j]);
        before += __builtin_amdgcn_mbcnt_hi((uint32_t)(b >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)b, 0u));
        total += (uint32_t)__popcll(b);
    }
    if (lane == 0) wave_count[wave] = total;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t sum = 0;
#pragma unroll
        for (uint32_t w = 0; w < kWaves; w++) sum += wave_count[w];
        block_base = sum ? atomicAdd(&a.counters[0], sum) : 0u;
    }
    __syncthreads();
    uint32_t at = block_base + before;
#pragma unroll
    for (uint32_t w = 0; w < kWaves; w++) at += w < wave ? wave_count[w] : 0u;
#pragma unroll
    for (uint32_t j = 0; j < kAbovePer; j++) {
        // (at < n whenever the counter started at 0: at most one slot per score)
        if (take[j] && at < a.n) a.cand[at] = make_uint2(e0 + j, (uint32_t)x[j]);
        at += take[j] ? 1u : 0u;
    }
}

}  // namespace

hipError_t launch_above(const AboveArgs& a, hipStream_t st) {
    if (a.n == 0) return hipSuccess;
    if (a.nviews > kAboveThreads) return hipErrorInvalidValue;   // (block 0 writes the views' header words)
    (void)ssa_launch((const void*)&above_select, dim3((a.n + kAboveBlock - 1) / kAboveBlock), dim3(kAboveThreads), 0,
                     st, a);
    return hipGetLastError();
}

}  // namespace ssa
