// Blank-frame skipping in front of the host beam decoders (amdspeech.h: amdspeech_ctc_blank_skip; host side: acoustic_model.py,
// config key decode_blank_skip).  No reference counterpart (an opt-in deviation).  Three plain launches, no kernel
// waits for another workgroup, no atomics.
//
//   bs_rows_kernel    one row of C logits per wavefront (C <= 1024, four rows per workgroup) or per 256-thread workgroup (C <= 4096),
//                     the row held in registers: lane l owns the units l, l + TPR, ... -- a unit is one 16-byte vector where
//                     C % 4 == 0 (rows of 320 B at C = 80 are then 16-byte aligned), one word otherwise.  The maximum and the sum of
//                     exp(x - max) meet in an xor butterfly (32, 16, 8, 4, 2, 1), and across the four waves of a workgroup through LDS
//                     in wave order: a fixed order, two runs give the same bits, and the order depends on C alone.  Lane 0 writes
//                     lpb (when asked for) and the flag byte skip[b][t]; a row at or past its utterance's length is not read.
//   bs_scan_kernel    one workgroup of BS_CHUNK threads per utterance walks time in chunks of BS_CHUNK frames, one frame per thread:
//                     keep[t] from the flags of t and t - 1 (the byte of t - 1 is read where it lies, so a chunk seam is no special
//                     case), the rank of a kept frame inside the chunk from a ballot and popcount per wave plus the four wave totals
//                     in LDS, and the count carried from chunk to chunk in a register.  Writes src_frame (-1 past the kept frames)
//                     and out_lengths.
//   bs_gather_kernel  one thread per 16-byte vector (C % 4 == 0) or word of out_logits [T][B][C]: row (j, b) copies row
//                     (src_frame[b][j], b) of logits, or is zero where src_frame is -1.
// Gathering inside the scan kernel would leave the copy of the whole tensor to B workgroups; as its own launch it runs over T * B
// rows on every compute unit.
#include "common.h"

#include <cmath>

namespace amdspeech {

constexpr int BS_THREADS = 256;             // rows and gather kernels
constexpr int BS_CHUNK = 256;               // frames per step of the scan kernel, one per thread
constexpr int BS_C_MAX = 4096;
constexpr int BS_WAVE_C_MAX = 1024;

typedef amdspeech_ctc_blank_skip_plan_info BlankSkipPlan;

#define BS_CHECK_SUPPORTED(cond, ...)                   \
    do {                                                \
        if (!(cond)) {                                  \
            ::amdspeech::set_error(__VA_ARGS__);        \
            return AMDSPEECH_EUNSUPPORTED;              \
        }                                               \
    } while (0)

// The one function that decides: the calls plan first and LAUNCH from the struct; amdspeech_ctc_blank_skip_plan returns the same
// struct.  No device is needed.
static int plan_blank_skip(int T, int B, int C, BlankSkipPlan* p) {
    AS_CHECK_ARG(T >= 1 && B >= 1, "ctc_blank_skip: bad shape (T %d, B %d): both must be at least 1", T, B);
    AS_CHECK_ARG(C >= 2, "ctc_blank_skip: C = %d is below 2 (a label and the blank)", C);
    BS_CHECK_SUPPORTED(C <= BS_C_MAX, "ctc_blank_skip: C = %d is above %d, the widest row the kernels hold in registers", C, BS_C_MAX);
    BS_CHECK_SUPPORTED((long)T * B * C < (1L << 31), "ctc_blank_skip: T * B * C = %ld does not stay below 2^31", (long)T * B * C);
    const long rows = (long)T * B;
    p->kernel = C <= BS_WAVE_C_MAX ? AMDSPEECH_BLANK_SKIP_KERNEL_WAVE : AMDSPEECH_BLANK_SKIP_KERNEL_BLOCK;
    const int tpr = p->kernel == AMDSPEECH_BLANK_SKIP_KERNEL_WAVE ? 64 : BS_THREADS;
    const int lo = p->kernel == AMDSPEECH_BLANK_SKIP_KERNEL_WAVE ? 4 : 8;
    int wpl = lo;
    while (wpl * tpr < C) wpl *= 2;
    p->words_per_lane = wpl;
    p->vec = C % 4 == 0 ? 4 : 1;
    p->c_max = wpl * tpr;                                           // the range of C on this very instantiation (per value of vec)
    p->c_min = wpl == lo ? (tpr == 64 ? 2 : BS_WAVE_C_MAX + 1) : wpl * tpr / 2 + 1;
    p->rows_threads = BS_THREADS;
    p->rows_per_workgroup = BS_THREADS / tpr;
    p->rows_grid = (int)((rows + p->rows_per_workgroup - 1) / p->rows_per_workgroup);
    p->t_chunk = BS_CHUNK;
    p->chunks = ceil_div(T, BS_CHUNK);
    p->scan_threads = BS_CHUNK;
    p->scan_grid = B;
    p->gather_threads = BS_THREADS;
    p->gather_grid = (int)((rows * C / p->vec + BS_THREADS - 1) / BS_THREADS);
    p->launches = 3;
    p->workspace_bytes = (int)align_up((size_t)rows, 256);          // one flag byte per frame, [B][T]
    return AMDSPEECH_OK;
}

template <int TPR>
__device__ __forceinline__ float bs_reduce(float v, bool is_max, float* lds) {
    for (int o = 32; o > 0; o >>= 1) {
        const float u = __shfl_xor(v, o, 64);
        v = is_max ? fmaxf(v, u) : v + u;
    }
    if (TPR > 64) {                                // one row per workgroup: the four waves' values through LDS, the same order in every thread
        const int wave = threadIdx.x >> 6;
        __syncthreads();                           // (the previous reduction's reads are over)
        if ((threadIdx.x & 63) == 0) lds[wave] = v;
        __syncthreads();
        v = lds[0];
        for (int k = 1; k < TPR / 64; ++k) v = is_max ? fmaxf(v, lds[k]) : v + lds[k];
    }
    return v;
}

// WPL words per lane, TPR threads per row, VEC: the lane's words come as 16-byte vectors (C % 4 == 0, a 16-byte aligned base)
template <int WPL, int TPR, bool VEC>
__global__ __launch_bounds__(BS_THREADS) void bs_rows_kernel(const float* __restrict__ logits, const int* __restrict__ lengths, int rows,
                                                             int T, int B, int C, float log_threshold,
                                                             unsigned char* __restrict__ flags, float* __restrict__ blank_logp) {
    __shared__ float red[BS_THREADS / 64];
    constexpr int RPW = BS_THREADS / TPR;
    const int sub = threadIdx.x / TPR, lane = threadIdx.x - sub * TPR;
    const int row = blockIdx.x * RPW + sub;
    if (row >= rows) return;                       // (a whole wave at TPR 64; never at TPR 256: one row per workgroup)
    const int t = row / B, b = row - t * B;
    int n = lengths[b];
    n = n < T ? n : T;
    if (t >= n) {                                  // uniform over the row's lanes: the row is not read
        if (lane == 0) {
            flags[(long)b * T + t] = 0;
            if (blank_logp) blank_logp[row] = 0.0f;
        }
        return;
    }
    const float* x_row = logits + (long)row * C;
    float x[WPL];
    if constexpr (VEC) {
#pragma unroll
        for (int i = 0; i < WPL / 4; ++i) {
            const int c = 4 * (lane + i * TPR);
            f32x4 q = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
            if (c < C) q = *reinterpret_cast<const f32x4*>(x_row + c);
            x[4 * i] = q.x; x[4 * i + 1] = q.y; x[4 * i + 2] = q.z; x[4 * i + 3] = q.w;
        }
    } else {
#pragma unroll
        for (int i = 0; i < WPL; ++i) {
            const int c = lane + i * TPR;
            x[i] = c < C ? x_row[c] : -INFINITY;
        }
    }
    const float xb = x_row[C - 1];
    float m = -INFINITY;
#pragma unroll
    for (int i = 0; i < WPL; ++i) m = fmaxf(m, x[i]);
    m = bs_reduce<TPR>(m, true, red);
    float s = 0.0f;
#pragma unroll
    for (int i = 0; i < WPL; ++i) s += x[i] == -INFINITY ? 0.0f : expf(x[i] - m);      // (a word past C, or a logit of -inf)
    s = bs_reduce<TPR>(s, false, red);
    if (lane == 0) {
        const float lpb = (xb - m) - logf(s);
        flags[(long)b * T + t] = lpb >= log_threshold ? 1 : 0;      // (a NaN compares false: the frame is kept)
        if (blank_logp) blank_logp[row] = lpb;
    }
}

__global__ __launch_bounds__(BS_CHUNK) void bs_scan_kernel(const unsigned char* __restrict__ flags, const int* __restrict__ lengths, int T,
                                                           int* __restrict__ src_frame, int* __restrict__ out_lengths) {
    __shared__ int wave_total[BS_CHUNK / 64];
    const int b = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    int n = lengths[b];
    n = n < T ? n : T;
    n = n > 0 ? n : 0;
    const unsigned char* f = flags + (long)b * T;
    int* src = src_frame + (long)b * T;
    int base = 0;                                                   // kept frames before this chunk (the same in every thread)
    for (int t0 = 0; t0 < n; t0 += BS_CHUNK) {
        const int t = t0 + tid;
        bool keep = false;
        if (t < n) keep = !(f[t] && t > 0 && f[t - 1]);             // of a run of skippable frames the first one stays
        const unsigned long long mask = __ballot(keep);
        const int before = __popcll(mask & ((1ull << lane) - 1ull));
        if (lane == 0) wave_total[wave] = __popcll(mask);
        __syncthreads();
        int offset = base, total = 0;
        for (int k = 0; k < BS_CHUNK / 64; ++k) {
            if (k < wave) offset += wave_total[k];
            total += wave_total[k];
        }
        if (keep) src[offset + before] = t;
        base += total;
        __syncthreads();                                            // (wave_total is the next chunk's too)
    }
    for (int j = base + tid; j < T; j += BS_CHUNK) src[j] = -1;
    if (tid == 0) out_lengths[b] = base;
}

template <bool VEC>
__global__ __launch_bounds__(BS_THREADS) void bs_gather_kernel(const float* __restrict__ logits, const int* __restrict__ src_frame, int T,
                                                               int B, int C, long units, float* __restrict__ out) {
    const long u = (long)blockIdx.x * BS_THREADS + threadIdx.x;
    if (u >= units) return;
    const int per_row = VEC ? C / 4 : C;
    const int row = (int)(u / per_row), col = (int)(u - (long)row * per_row);
    const int j = row / B, b = row - j * B;
    const int t = src_frame[(long)b * T + j];
    if constexpr (VEC) {
        f32x4 q = {0.0f, 0.0f, 0.0f, 0.0f};
        if (t >= 0) q = reinterpret_cast<const f32x4*>(logits + ((long)t * B + b) * C)[col];
        reinterpret_cast<f32x4*>(out)[u] = q;
    } else {
        out[u] = t >= 0 ? logits[((long)t * B + b) * C + col] : 0.0f;
    }
}

template <int WPL, int TPR>
static void launch_rows(hipStream_t s, const BlankSkipPlan& p, const float* logits, const int* lengths, int T, int B, int C,
                        float log_threshold, unsigned char* flags, float* blank_logp) {
    if (p.vec == 4)
        hipLaunchKernelGGL((bs_rows_kernel<WPL, TPR, true>), dim3(p.rows_grid), dim3(p.rows_threads), 0, s, logits, lengths, T * B, T, B, C,
                           log_threshold, flags, blank_logp);
    else
        hipLaunchKernelGGL((bs_rows_kernel<WPL, TPR, false>), dim3(p.rows_grid), dim3(p.rows_threads), 0, s, logits, lengths, T * B, T, B, C,
                           log_threshold, flags, blank_logp);
}

}  // namespace amdspeech

using namespace amdspeech;

extern "C" int amdspeech_ctc_blank_skip_plan(int T, int B, int C, amdspeech_ctc_blank_skip_plan_info* out) {
    AS_CHECK_ARG(out != nullptr, "ctc_blank_skip_plan: null output");
    return plan_blank_skip(T, B, C, out);
}

extern "C" size_t amdspeech_ctc_blank_skip_workspace_bytes(int T, int B, int C) {
    BlankSkipPlan p;
    if (plan_blank_skip(T, B, C, &p)) return 0;
    return (size_t)p.workspace_bytes;
}

extern "C" int amdspeech_ctc_blank_skip(void* stream, const float* logits, const int* lengths, int T, int B, int C, float log_threshold,
                                        float* out_logits, int* out_lengths, int* src_frame, float* blank_logp, void* ws) {
    BlankSkipPlan p;
    if (int rc = plan_blank_skip(T, B, C, &p)) return rc;
    AS_CHECK_ARG(std::isfinite(log_threshold) && log_threshold <= 0.0f,
                 "ctc_blank_skip: log_threshold %g must be finite and at most 0 (the log of a probability)", (double)log_threshold);
    AS_CHECK_ARG(logits && lengths && out_logits && out_lengths && src_frame && ws, "ctc_blank_skip: null pointer");
    {
        const uintptr_t a = reinterpret_cast<uintptr_t>(logits), o = reinterpret_cast<uintptr_t>(out_logits), nb = (uintptr_t)T * B * C * 4;
        AS_CHECK_ARG(a + nb <= o || o + nb <= a, "ctc_blank_skip: out_logits overlaps logits (rows move forward in time: the call does not work in place)");
    }
    AS_CHECK_ARG(p.vec == 1 || ((reinterpret_cast<uintptr_t>(logits) | reinterpret_cast<uintptr_t>(out_logits)) & 15) == 0,
                 "ctc_blank_skip: logits and out_logits must be 16-byte aligned when C is a multiple of 4");
    hipStream_t s = static_cast<hipStream_t>(stream);
    unsigned char* flags = static_cast<unsigned char*>(ws);
    const bool wave = p.kernel == AMDSPEECH_BLANK_SKIP_KERNEL_WAVE;
#define BS_CASE(WPL, TPR) launch_rows<WPL, TPR>(s, p, logits, lengths, T, B, C, log_threshold, flags, blank_logp)
    switch (p.words_per_lane) {
        case 4: BS_CASE(4, 64); break;
        case 8: if (wave) BS_CASE(8, 64); else BS_CASE(8, 256); break;
        case 16: if (wave) BS_CASE(16, 64); else BS_CASE(16, 256); break;
        default: AS_CHECK_ARG(false, "ctc_blank_skip: no kernel for %d words per lane", p.words_per_lane);
    }
#undef BS_CASE
    AS_CHECK_LAUNCH();
    hipLaunchKernelGGL(bs_scan_kernel, dim3(p.scan_grid), dim3(p.scan_threads), 0, s, flags, lengths, T, src_frame, out_lengths);
    AS_CHECK_LAUNCH();
    const long units = (long)T * B * C / p.vec;
    if (p.vec == 4)
        hipLaunchKernelGGL((bs_gather_kernel<true>), dim3(p.gather_grid), dim3(p.gather_threads), 0, s, logits, src_frame, T, B, C, units,
                           out_logits);
    else
        hipLaunchKernelGGL((bs_gather_kernel<false>), dim3(p.gather_grid), dim3(p.gather_threads), 0, s, logits, src_frame, T, B, C, units,
                           out_logits);
    AS_CHECK_LAUNCH();
    return AMDSPEECH_OK;
}
