// Host-side row lengths on their way into a kernel (frame_stack.hip, feature_norm.hip, frontend.hip).  Up to ROW_ARGS_MAX rows travel
// as KERNEL ARGUMENTS: no pageable host-to-device copy and no stream synchronisation on the hot path.  A wider batch goes through
// device memory, and each caller's kernels are compiled for both routes (a bool template parameter, read through row_arg).
#pragma once

#include "common.h"

#include <type_traits>

namespace amdspeech {

constexpr int ROW_ARGS_MAX = 256;
struct RowArgs { int v[ROW_ARGS_MAX]; };

// Row b's length: from the argument block (BY_ARG) or from the device vector.
template <bool BY_ARG>
static __device__ __forceinline__ int row_arg(const RowArgs& args, const int* dev, int b) {
    return BY_ARG ? args.v[b] : dev[b];
}

// Runs launch(by_arg, args, dev) -> hipError_t with the B host values of `rows` in reach of its kernels; by_arg is std::true_type
// (the values are in `args`, dev is null) or std::false_type (they are at `dev`, `args` is zeros).  More rows than the block holds
// go through a device buffer of the call's own, and the call waits for the kernels before it gives the buffer back; the launch
// or synchronise error is reported before the free's.
template <class Launch>
static int with_row_args(hipStream_t s, const int* rows, int B, Launch&& launch) {
    RowArgs args;
    if (B <= ROW_ARGS_MAX) {
        for (int b = 0; b < ROW_ARGS_MAX; ++b) args.v[b] = b < B ? rows[b] : 0;
        AS_CHECK_HIP(launch(std::true_type{}, args, static_cast<const int*>(nullptr)));
        return AMDSPEECH_OK;
    }
    for (int b = 0; b < ROW_ARGS_MAX; ++b) args.v[b] = 0;
    int* dev = nullptr;
    AS_CHECK_HIP(hipMalloc(reinterpret_cast<void**>(&dev), (size_t)B * sizeof(int)));
    hipError_t e = hipMemcpyAsync(dev, rows, (size_t)B * sizeof(int), hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = launch(std::false_type{}, args, static_cast<const int*>(dev));
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    const hipError_t ef = hipFree(dev);
    AS_CHECK_HIP(e);
    AS_CHECK_HIP(ef);
    return AMDSPEECH_OK;
}

// Host-side int vectors that kernels read from a WORKSPACE (frontend.hip, augment.hip) reach the device as KERNEL ARGUMENTS of a
// one-block kernel (no pageable H2D copy, no stream synchronisation on the hot path), two values per row of the block above a launch.
struct MetaArg { int v[2 * ROW_ARGS_MAX]; };
static __global__ void write_meta_kernel(MetaArg m, int* dst, int n) {
    for (int i = threadIdx.x; i < n; i += blockDim.x) dst[i] = m.v[i];
}
// dst[0 .. count) = src[0 .. count), stream-ordered: one launch per 2 * ROW_ARGS_MAX values
static inline void write_ints(hipStream_t s, int* dst, const int* src, int count) {
    for (int i0 = 0; i0 < count; i0 += 2 * ROW_ARGS_MAX) {
        MetaArg m;
        const int cnt = count - i0 < 2 * ROW_ARGS_MAX ? count - i0 : 2 * ROW_ARGS_MAX;
        for (int i = 0; i < cnt; ++i) m.v[i] = src[i0 + i];
        hipLaunchKernelGGL(write_meta_kernel, dim3(1), dim3(256), 0, s, m, dst + i0, cnt);
    }
}

}  // namespace amdspeech
