// Low frame rate input: `stack` consecutive front-end frames concatenated into one model frame, every `skip`-th one kept
// (amdspeech.h: amdspeech_frame_stack).  Followed by the model's input Linear this is a strided 1-D convolution over time; it divides
// the number of frames of everything behind it by `skip`.  No reference counterpart (an opt-in deviation).
//
//   out[j][b][i * D + d] = x[j * skip + i][b][d]   if j * skip + i < min(n_b, t_in),   0 otherwise
//
// A copy: bandwidth-bound (5 MB read, 5 MB written at the headline shape), so the kernel is plain 16-byte vector loads and stores
// under a grid-stride loop, no LDS, no atomics.  The words travel as unsigned integers: whatever bit pattern the front end wrote
// (-0.0, denormals, infinities, NaN payloads) arrives unchanged.  The kernel masks by the row's own length and never reads a
// source frame at or past it, so what the source holds there does not matter; it writes EVERY word of `out`.
#include "row_args.h"

namespace amdspeech {

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

constexpr int FS_THREADS = 256;
constexpr int FS_MAX_WGS = 2048;          // a streaming kernel: cap the grid and stride the rest
constexpr int FS_MAX_FACTOR = 16;         // stack, skip
constexpr int FS_MAX_WIDTH = 4096;        // stack * D

// Lanes that share one (model frame, row) item: the smallest power of two that covers its `units` vector words, at most a workgroup.
static __host__ __device__ inline int fs_lanes_per_item(int units) {
    int l = 1;
    while (l < units && l < FS_THREADS) l *= 2;
    return l;
}

// One item = the d_out words of out[j][b]; FS_THREADS / lanes items per workgroup and pass.  V: words per lane and access (4 or 1).
template <int V, bool LEN_ARG>
__global__ __launch_bounds__(FS_THREADS) void frame_stack_kernel(const unsigned* __restrict__ x, unsigned* __restrict__ out,
                                                                 RowArgs len_arg, const int* __restrict__ len_dev, int B, int D,
                                                                 int t_in, int stack, int skip, int t_out, int lanes) {
    const int dv = D / V;                          // vector words per source frame
    const int units = stack * dv;                  // ... per item
    const int per_wg = FS_THREADS / lanes;
    const int sub = threadIdx.x / lanes, lane = threadIdx.x - sub * lanes;
    const long n_items = (long)t_out * B;
    for (long item = (long)blockIdx.x * per_wg + sub; item < n_items; item += (long)gridDim.x * per_wg) {
        const int j = (int)(item / B), b = (int)(item - (long)j * B);
        int n = row_arg<LEN_ARG>(len_arg, len_dev, b);
        n = n < t_in ? n : t_in;                   // (the front end's counts are not clipped to its t_max)
        const int t0 = j * skip;
        unsigned* o = out + item * ((long)units * V);
        for (int u = lane; u < units; u += lanes) {
            const int i = u / dv, w = u - i * dv;
            const int t = t0 + i;
            const bool live = t < n;
            const unsigned* src = x + ((long)t * B + b) * D + (long)w * V;
            if (V == 4) {
                u32x4 v = {0u, 0u, 0u, 0u};
                if (live) v = *reinterpret_cast<const u32x4*>(src);
                *reinterpret_cast<u32x4*>(o + (long)u * 4) = v;
            } else {
                o[u] = live ? *src : 0u;
            }
        }
    }
}

// ---- the plan: the launch geometry as plain numbers (amdspeech.h: amdspeech_frame_stack_plan_info).  amdspeech_frame_stack plans
// first and LAUNCHES from the struct; amdspeech_frame_stack_plan returns the same struct.  No device is needed.
typedef amdspeech_frame_stack_plan_info FsPlan;

static int plan_frame_stack(int B, int D, int t_in, int stack, int skip, FsPlan* p) {
    AS_CHECK_ARG(B > 0 && D > 0 && t_in > 0, "frame_stack: bad shape (B %d, D %d, t_in %d)", B, D, t_in);
    AS_CHECK_ARG(stack >= 1 && stack <= FS_MAX_FACTOR, "frame_stack: stack %d outside 1 .. %d", stack, FS_MAX_FACTOR);
    AS_CHECK_ARG(skip >= 1 && skip <= FS_MAX_FACTOR, "frame_stack: skip %d outside 1 .. %d", skip, FS_MAX_FACTOR);
    AS_CHECK_ARG((long)stack * D <= FS_MAX_WIDTH, "frame_stack: stack * D = %ld exceeds %d", (long)stack * D, FS_MAX_WIDTH);
    p->t_out = ceil_div(t_in, skip);
    p->d_out = stack * D;
    p->vec = D % 4 == 0 ? 4 : 1;
    const int per_wg = FS_THREADS / fs_lanes_per_item(p->d_out / p->vec);
    const long wgs = ((long)p->t_out * B + per_wg - 1) / per_wg;
    p->workgroups = (int)(wgs < FS_MAX_WGS ? wgs : FS_MAX_WGS);
    p->meta_by_copy = B > ROW_ARGS_MAX ? 1 : 0;
    return AMDSPEECH_OK;
}

static int run_frame_stack(hipStream_t s, const float* x, const int* n_frames, int B, int D, int t_in, int stack, int skip,
                           float* out, int* n_out) {
    AS_CHECK_ARG(x && n_frames && out && n_out, "frame_stack: null pointer");
    FsPlan pl;
    if (int rc = plan_frame_stack(B, D, t_in, stack, skip, &pl)) return rc;
    const uintptr_t xa = reinterpret_cast<uintptr_t>(x), oa = reinterpret_cast<uintptr_t>(out);
    const uintptr_t xe = xa + (uintptr_t)t_in * B * D * 4, oe = oa + (uintptr_t)pl.t_out * B * pl.d_out * 4;
    AS_CHECK_ARG(xe <= oa || oe <= xa, "frame_stack: x and out overlap");
    AS_CHECK_ARG(pl.vec == 1 || ((xa | oa) & 15) == 0, "frame_stack: x and out must be 16-byte aligned when D is a multiple of 4");
    for (int b = 0; b < B; ++b)
        AS_CHECK_ARG(n_frames[b] >= 0, "frame_stack: n_frames[%d] = %d is negative", b, n_frames[b]);
    for (int b = 0; b < B; ++b) n_out[b] = ceil_div(n_frames[b], skip);

    const unsigned* xs = reinterpret_cast<const unsigned*>(x);
    unsigned* os = reinterpret_cast<unsigned*>(out);
    const int lanes = fs_lanes_per_item(pl.d_out / pl.vec);
    // (more rows than the argument block holds: with_row_args waits for the kernel, as the front end's wide-batch path does)
    return with_row_args(s, n_frames, B, [&](auto by_arg, const RowArgs& la, const int* d_len) {
        constexpr bool LEN_ARG = decltype(by_arg)::value;
        if (pl.vec == 4)
            hipLaunchKernelGGL((frame_stack_kernel<4, LEN_ARG>), dim3(pl.workgroups), dim3(FS_THREADS), 0, s, xs, os, la, d_len, B, D, t_in,
                               stack, skip, pl.t_out, lanes);
        else
            hipLaunchKernelGGL((frame_stack_kernel<1, LEN_ARG>), dim3(pl.workgroups), dim3(FS_THREADS), 0, s, xs, os, la, d_len, B, D, t_in,
                               stack, skip, pl.t_out, lanes);
        return hipGetLastError();
    });
}

}  // namespace amdspeech

using namespace amdspeech;

extern "C" int amdspeech_frame_stack_num_frames(int n_frames, int skip) {
    if (n_frames < 0 || skip < 1 || skip > FS_MAX_FACTOR) return AMDSPEECH_EINVAL;
    return ceil_div(n_frames, skip);
}

extern "C" int amdspeech_frame_stack_plan(int B, int D, int t_in, int stack, int skip, amdspeech_frame_stack_plan_info* out) {
    AS_CHECK_ARG(out != nullptr, "frame_stack_plan: null output");
    return plan_frame_stack(B, D, t_in, stack, skip, out);
}

extern "C" int amdspeech_frame_stack(void* stream, const float* x, const int* n_frames, int B, int D, int t_in, int stack, int skip,
                                     float* out, int* n_out) {
    return run_frame_stack(static_cast<hipStream_t>(stream), x, n_frames, B, D, t_in, stack, skip, out, n_out);
}
