// SpecAugment: frequency and time masks on a training mini-batch's features, in place (amdspeech.h: amdspeech_spec_augment).
// No reference counterpart (an opt-in deviation).  The features never visit the host as a time-frequency tensor, so
// the masks are drawn and applied on the device; the input needs no gradient, so there is no backward kernel.
//
//   x[t][b][c] = +0.0f   if t < n_b and (c % P lies in a frequency span of row b  or  t lies in a time span of row b),   n_b = min(len_b, T)
//
// WRITE-ONLY: the operation is in place and the mask value is a constant, so the kernel reads the lengths and its arguments,
// computes the row's spans and stores zeros to the masked words -- it loads nothing from x and stores to no other word (frames at
// or past n_b included).  At the headline shape that is under 1 MB of stores: launch-bound.  Plain vector and single-word stores
// under a grid-stride loop, no LDS, no atomics.  Every thread of an item draws its row's spans itself (at most 24 masks x 2 draws
// of two 32-bit hashes), so an item's lanes need no exchange; the draws, not the stores, are the kernel's work (their multiplies
// run at a quarter of the vector rate), which is why an item gets only a quarter of the lanes its frame has stores: each lane
// then makes up to SA_STORES_PER_LANE of them and the hashing is shared by four times fewer threads.
//
// The draws are integer arithmetic only (random24, common.h): the host function amdspeech_spec_augment_spans calls the SAME
// sa_span the kernel calls, and a numpy restatement agrees with both exactly.
#include "common.h"


namespace amdspeech {

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

constexpr int SA_THREADS = 256;
constexpr int SA_MAX_WGS = 2048;          // a streaming kernel: cap the grid and stride the rest
constexpr int SA_STORES_PER_LANE = 4;     // stores of a whole (time-masked) frame one lane makes, when the frame has that many
constexpr int SA_MAX_WIDTH = 4096;        // W
constexpr int SA_MAX_FREQ_MASKS = 8;
constexpr int SA_MAX_TIME_MASKS = 16;
constexpr uint32_t SA_STREAM = 0x5A000000u;      // + 2 * kind + which

typedef amdspeech_spec_augment_desc SaDesc;
typedef amdspeech_spec_augment_plan_info SaPlan;
struct SaSpan { int start, width; };

// Mask m of a kind (0 frequency, 1 time) of row b with n = min(len_b, T) >= 0 frames.  64-bit products of a 24-bit draw.
static __host__ __device__ inline SaSpan sa_span(const SaDesc& d, int kind, int row, int m, int n) {
    const uint32_t idx = (uint32_t)row * 64u + (uint32_t)m;
    int wmax, extent;
    if (kind == 0) {
        wmax = d.freq_width < d.period ? d.freq_width : d.period;
        extent = d.period;
    } else {
        const long cap = (long)n * d.time_permille / 1000;
        wmax = d.time_width < cap ? d.time_width : (int)cap;
        extent = n;
    }
    SaSpan s;
    s.width = (int)(((uint64_t)random24(d.seed, SA_STREAM + 2u * kind, idx) * (uint64_t)(wmax + 1)) >> 24);
    s.start = (int)(((uint64_t)random24(d.seed, SA_STREAM + 2u * kind + 1u, idx) * (uint64_t)(extent - s.width + 1)) >> 24);
    return s;
}

// Lanes that share one (frame, row) item: the smallest power of two that covers a whole frame's `units` stores at
// SA_STORES_PER_LANE each, at most a workgroup.
static __host__ __device__ inline int sa_lanes_per_item(int units) {
    int l = 1;
    while (l * SA_STORES_PER_LANE < units && l < SA_THREADS) l *= 2;
    return l;
}

// One item = the W words of x[t][b]; SA_THREADS / lanes items per workgroup and pass.  V: words per store of a time-masked frame.
template <int V>
__global__ __launch_bounds__(SA_THREADS) void spec_augment_kernel(unsigned* __restrict__ x, const int* __restrict__ len, int T, int B,
                                                                  int W, SaDesc d, int lanes) {
    const int per_wg = SA_THREADS / lanes;
    const int sub = threadIdx.x / lanes, lane = threadIdx.x - sub * lanes;
    const int reps = W / d.period;
    const unsigned n_items = (unsigned)T * (unsigned)B;            // (the plan refuses T * B >= 2^31)
    for (unsigned item = blockIdx.x * per_wg + sub; item < n_items; item += gridDim.x * per_wg) {
        const int t = (int)(item / (unsigned)B), b = (int)(item - (unsigned)t * (unsigned)B);
        int n = len[b];
        n = n < T ? n : T;
        if (t >= n) continue;                      // past the row's length (or an empty row): nothing is written
        unsigned* row = x + (long)item * W;
        bool in_time = false;
        for (int m = 0; m < d.time_masks; ++m) {
            const SaSpan s = sa_span(d, 1, b, m, n);
            in_time |= t >= s.start && t < s.start + s.width;
        }
        if (in_time) {                             // the whole frame
            if (V == 4) {
                const u32x4 z = {0u, 0u, 0u, 0u};
                for (int u = lane; u < W / 4; u += lanes) *reinterpret_cast<u32x4*>(row + (long)u * 4) = z;
            } else {
                for (int u = lane; u < W; u += lanes) row[u] = 0u;
            }
            continue;
        }
        for (int m = 0; m < d.freq_masks; ++m) {   // the span's bins in each of the W / P repetitions: any word offset
            const SaSpan s = sa_span(d, 0, b, m, n);
            const int words = reps * s.width;
            for (int i = lane; i < words; i += lanes) {
                const int r = i / s.width, k = i - r * s.width;
                row[r * d.period + s.start + k] = 0u;
            }
        }
    }
}

static int check_policy(const SaDesc* d) {
    AS_CHECK_ARG(d != nullptr, "spec_augment: null policy");
    AS_CHECK_ARG(d->period >= 1 && d->period <= SA_MAX_WIDTH, "spec_augment: period %d outside 1 .. %d", d->period, SA_MAX_WIDTH);
    AS_CHECK_ARG(d->freq_masks >= 0 && d->freq_masks <= SA_MAX_FREQ_MASKS, "spec_augment: freq_masks %d outside 0 .. %d",
                 d->freq_masks, SA_MAX_FREQ_MASKS);
    AS_CHECK_ARG(d->time_masks >= 0 && d->time_masks <= SA_MAX_TIME_MASKS, "spec_augment: time_masks %d outside 0 .. %d",
                 d->time_masks, SA_MAX_TIME_MASKS);
    AS_CHECK_ARG(d->freq_width >= 0 && d->freq_width <= d->period, "spec_augment: freq_width %d outside 0 .. period %d",
                 d->freq_width, d->period);
    AS_CHECK_ARG(d->time_width >= 0, "spec_augment: time_width %d is negative", d->time_width);
    AS_CHECK_ARG(d->time_permille >= 0 && d->time_permille <= 1000, "spec_augment: time_permille %d outside 0 .. 1000",
                 d->time_permille);
    return AMDSPEECH_OK;
}

// ---- the plan: the launch geometry as plain numbers (amdspeech.h: amdspeech_spec_augment_plan_info).  amdspeech_spec_augment
// plans first and LAUNCHES from the struct; amdspeech_spec_augment_plan returns the same struct (for an aligned x).  No device.
static int plan_spec_augment(int T, int B, int W, const SaDesc* d, bool aligned16, SaPlan* p) {
    AS_CHECK_ARG(T > 0 && B > 0 && (long)T * B < (1L << 31), "spec_augment: bad shape (T %d, B %d)", T, B);
    AS_CHECK_ARG(W >= 1 && W <= SA_MAX_WIDTH, "spec_augment: W %d outside 1 .. %d", W, SA_MAX_WIDTH);
    if (int rc = check_policy(d)) return rc;
    AS_CHECK_ARG(d->period <= W && W % d->period == 0, "spec_augment: period %d does not divide W %d", d->period, W);
    p->vec = (W % 4 == 0 && aligned16) ? 4 : 1;
    p->lanes = sa_lanes_per_item(W / p->vec);
    p->items_per_workgroup = SA_THREADS / p->lanes;
    p->reps = W / d->period;
    const bool freq_on = d->freq_masks > 0 && d->freq_width > 0;
    const bool time_on = d->time_masks > 0 && d->time_width > 0 && d->time_permille > 0;
    const long wgs = ((long)T * B + p->items_per_workgroup - 1) / p->items_per_workgroup;
    p->workgroups = (freq_on || time_on) ? (int)(wgs < SA_MAX_WGS ? wgs : SA_MAX_WGS) : 0;
    return AMDSPEECH_OK;
}

static int run_spec_augment(hipStream_t s, float* x, const int* lengths, int T, int B, int W, const SaDesc* d) {
    AS_CHECK_ARG(x && lengths && d, "spec_augment: null pointer");
    SaPlan pl;
    if (int rc = plan_spec_augment(T, B, W, d, (reinterpret_cast<uintptr_t>(x) & 15) == 0, &pl)) return rc;
    if (pl.workgroups == 0) return AMDSPEECH_OK;                  // neither kind can mask anything
    unsigned* xs = reinterpret_cast<unsigned*>(x);
    if (pl.vec == 4)
        hipLaunchKernelGGL((spec_augment_kernel<4>), dim3(pl.workgroups), dim3(SA_THREADS), 0, s, xs, lengths, T, B, W, *d, pl.lanes);
    else
        hipLaunchKernelGGL((spec_augment_kernel<1>), dim3(pl.workgroups), dim3(SA_THREADS), 0, s, xs, lengths, T, B, W, *d, pl.lanes);
    AS_CHECK_LAUNCH();
    return AMDSPEECH_OK;
}

}  // namespace amdspeech

using namespace amdspeech;

extern "C" int amdspeech_spec_augment_spans(const amdspeech_spec_augment_desc* desc, int row, int n, int* spans) {
    AS_CHECK_ARG(desc && spans, "spec_augment_spans: null pointer");
    if (int rc = check_policy(desc)) return rc;
    AS_CHECK_ARG(row >= 0 && n >= 0, "spec_augment_spans: negative row %d or length %d", row, n);
    int* o = spans;
    for (int kind = 0; kind < 2; ++kind)
        for (int m = 0; m < (kind == 0 ? desc->freq_masks : desc->time_masks); ++m) {
            const SaSpan s = sa_span(*desc, kind, row, m, n);
            *o++ = s.start;
            *o++ = s.width;
        }
    return AMDSPEECH_OK;
}

extern "C" int amdspeech_spec_augment_plan(int T, int B, int W, const amdspeech_spec_augment_desc* desc,
                                           amdspeech_spec_augment_plan_info* out) {
    AS_CHECK_ARG(out != nullptr, "spec_augment_plan: null output");
    return plan_spec_augment(T, B, W, desc, true, out);
}

extern "C" int amdspeech_spec_augment(void* stream, float* x, const int* lengths, int T, int B, int W,
                                      const amdspeech_spec_augment_desc* desc) {
    return run_spec_augment(static_cast<hipStream_t>(stream), x, lengths, T, B, W, desc);
}
