// launch.h -- typed launch helpers: a kernel launch that takes its arguments
// by reference and builds hipLaunchKernel's pointer array, and the memset the
// launch wrappers in the .hip files issue beside their kernels.
#pragma once
#include <hip/hip_runtime.h>

namespace ssa {

template <class... A>
hipError_t ssa_launch(const void* func, dim3 grid, dim3 block, size_t lds, hipStream_t st, const A&... a) {
    void* p[] = {(void*)&a..., nullptr};
    return hipLaunchKernel(func, grid, block, p, lds, st);
}

inline hipError_t op_set(void* dst, int value, size_t bytes, hipStream_t st) {
    return hipMemsetAsync(dst, value, bytes, st);
}

}  // namespace ssa
