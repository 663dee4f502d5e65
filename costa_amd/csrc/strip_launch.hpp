// The host launch of the strip kernel families (convert_kernels.hip, tri_kernels.hip,
// half_kernels.hip, fp8_kernels.hip, scaled_kernels.hip, mx_kernels.hip): each runs a work list built by
// build_strip_work (strip_work.hpp), one workgroup per work item, on a kernel whose first two
// arguments are the device array of ops and the work items.  Internal to the including file.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "engine.hpp"

namespace costa {
namespace engine {
namespace {

// KERNEL(d_ops, d_work + offset, args...) over the whole list, at most 2^30 workgroups of `threads`
// per launch.  LDS_BYTES is the kernel's staged tile: copy-only lists take none (more workgroups
// per CU); a tile over the default dynamic-LDS limit of 64 KiB is allowed once per kernel.  Throws
// "<family> kernel launch failed: ..." when a launch was refused.
template <auto KERNEL, size_t LDS_BYTES, typename Op, typename... Args>
void launch_strip(const char* family, int threads, const strip_list& l, hipStream_t stream, const Op* d_ops,
                  const uint64_t* d_work, Args... args) {
    const int64_t max_grid = 1LL << 30;
    const size_t lds = l.any_transpose ? LDS_BYTES : 0;
    if constexpr (LDS_BYTES > 64 * 1024) {
        static const bool once = [] {
            (void)hipFuncSetAttribute(reinterpret_cast<const void*>(KERNEL),
                                      hipFuncAttributeMaxDynamicSharedMemorySize, int(LDS_BYTES));
            return true;
        }();
        (void)once;
    }
    for (int64_t off = 0; off < l.n_items; off += max_grid) {
        const int64_t m = std::min(max_grid, l.n_items - off);
        hipLaunchKernelGGL(KERNEL, dim3(unsigned(m)), dim3(unsigned(threads)), lds, stream, d_ops, d_work + off,
                           args...);
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess)
        throw error(COSTA_ERR_HIP, std::string(family) + " kernel launch failed: " + hipGetErrorString(e));
}

}  // namespace
}  // namespace engine
}  // namespace costa
