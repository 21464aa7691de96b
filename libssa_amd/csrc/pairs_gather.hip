// pairs_gather.hip -- pairs_gather_kernel: packs one group of 64 pairs per
// workgroup into pairs.h's lane-interleaved layout, from sequence pools that
// lie in device memory (layout: pairs.h; arguments: pairs_gather.h; host
// side: pairs.cpp).
//
// Lane l of every wave owns pair l of the group.  It reads its own sequence
// front to back -- a stream per lane, at whatever byte the sequence starts --
// and each store instruction writes one whole 64-lane row of the output, the
// row pairs_kernel later loads with one instruction.
//
// gather_rows (gather_rows.h) is shared with hits_gather.hip.
#include "gather_rows.h"
#include "launch.h"
#include "pairs_gather.h"

namespace ssa {
namespace {

__global__ void __launch_bounds__(64 * kWaves) pairs_gather_kernel(const GatherArgs a) {
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t g = blockIdx.x;
    const PairsGroup G = a.groups[g];
    const PairsDesc D = a.desc[(size_t)g * 64 + lane];
    if (wave == 0) a.lens[(size_t)g * 64 + lane] = make_uint2(D.qlen, D.dlen);
    gather_rows(a.qpool, D.q_start, D.qlen, a.qres + ((size_t)G.q_row * 64 + lane), G.nstrips * 2, wave);
    gather_rows(a.dpool, D.d_start, D.dlen, a.tres + ((size_t)G.t_row * 64 + lane), G.ncb, wave);
}

}  // namespace

hipError_t launch_pairs_gather(const GatherArgs& a, hipStream_t st) {
    if (a.ngroups == 0) return hipSuccess;
    (void)ssa_launch((const void*)&pairs_gather_kernel, dim3(a.ngroups), dim3(64 * kWaves), 0, st, a);
    return hipGetLastError();
}

}  // namespace ssa
