// Lookahead (row) convolution above the top layer of a unidirectional LSTM stack (amdspeech.h: amdspeech_lookahead_fwd / _bwd): a
// depth-wise filter over the next `context` frames, one weight per future frame and hidden unit (Deep Speech 2).  No reference
// counterpart (an opt-in deviation); off at context 0, where no caller makes these calls.
//
//   Lb = min(lengths[b], T)
//   y[t][b][h]  = sum_{j = 0 .. context, t + j < Lb} w[j][h] * x[t + j][b][h]       t < Lb,  0 past it
//   dx[t][b][h] = sum_{j = 0 .. context, t - j >= 0} w[j][h] * dy[t - j][b][h]      t < Lb,  0 past it
//   dw[j][h]   += sum_b sum_{t, t + j < Lb} dy[t][b][h] * x[t + j][b][h]
//
// Bandwidth-bound, so every kernel is the same walk: a lane owns V (4 or 1) neighbouring hidden units of one row b -- the lanes of a
// 64-thread workgroup run along the contiguous [B][H] frame, 1 KiB per wave and load -- and walks one chunk of `t_chunk` frames in
// blocks of LA_U.  Per block it issues LA_U independent global loads (the frames that ENTER the window), parks them in a ring of
// context + LA_U frames in LDS, [slot][lane] so that a lane only ever touches its own words (no barrier anywhere, no bank conflict),
// and forms LA_U outputs from the ring.  Each frame is loaded from memory once per chunk; what a chunk re-reads is its halo of
// `context` frames, which the plan keeps at or under a quarter of the chunk.  The weights of the lane's units sit beside the ring.
//   lookahead_conv_kernel<V, +1>   y from x: the window runs forward from t; taps at or past Lb are neither read nor added
//   lookahead_conv_kernel<V, -1>   dx from dy: the window runs backward from t; taps before frame 0 are skipped
//   lookahead_dw_kernel<V>         the forward walk over x with dy[t] of the block in registers: context + 1 running sums per lane in
//                                  LDS (where the other kernel keeps the weights), one partial [context + 1][H] tile per (chunk, row)
//                                  into the workspace -- written in every word, so the workspace needs no fill
//   lookahead_dw_reduce_kernel     dw[j][h] += the partials: LA_SLICES threads per element each sum a contiguous run of partials in
//                                  index order, the slices meet in LDS and are added in slice order, then one add into dw
// Every output is ONE chain of fmaf in ascending j (dw: ascending t) that starts from a product; there is no atomic anywhere, so two
// runs give the same bits whatever else the chip is doing.  Frames of x / dy at or past Lb are never loaded; y and dx are written in
// every element.
#include "common.h"

#include <initializer_list>

namespace amdspeech {

constexpr int LA_THREADS = 64;            // one wave: a lane's ring is private, so nothing is gained from a wider workgroup
constexpr int LA_U = 8;                   // frames per block = independent loads in flight per lane
constexpr int LA_MAX_CONTEXT = 32;
constexpr int LA_TARGET_WGS = 1024;       // four waves per CU when the chunk floor allows it
constexpr int LA_HALO_FACTOR = 4;         // t_chunk >= 4 * context: a chunk re-reads at most a quarter of its own length
constexpr int LA_SLICES = 8;              // second stage of dw: threads per element
constexpr int LA_RED_COLS = 32;           // ... and elements per workgroup (256 threads)

typedef amdspeech_lookahead_plan_info LaPlan;

template <int V> struct LaVec;
template <> struct LaVec<4> {
    typedef f32x4 type;
    static __device__ inline f32x4 zero() { return f32x4{0.f, 0.f, 0.f, 0.f}; }
    static __device__ inline f32x4 mul(f32x4 a, f32x4 b) { return a * b; }      // (one rounding per component, as fmaf's start value)
    static __device__ inline f32x4 fma(f32x4 a, f32x4 b, f32x4 c) {
        return f32x4{fmaf(a.x, b.x, c.x), fmaf(a.y, b.y, c.y), fmaf(a.z, b.z, c.z), fmaf(a.w, b.w, c.w)};
    }
};
template <> struct LaVec<1> {
    typedef float type;
    static __device__ inline float zero() { return 0.f; }
    static __device__ inline float mul(float a, float b) { return a * b; }
    static __device__ inline float fma(float a, float b, float c) { return fmaf(a, b, c); }
};

// What every kernel of the walk knows about its lane.
struct LaLane {
    long col;          // first word of the lane inside a [B][H] frame
    int h, b, Lb;
    bool active;
};

static __device__ inline LaLane la_lane(const int* __restrict__ lengths, int T, int B, int H, int V) {
    LaLane l;
    const long q = (long)blockIdx.x * LA_THREADS + threadIdx.x;
    l.col = q * V;
    l.active = l.col < (long)B * H;
    l.b = l.active ? (int)(l.col / H) : 0;
    l.h = l.active ? (int)(l.col - (long)l.b * H) : 0;
    int n = l.active ? lengths[l.b] : 0;
    n = n < T ? n : T;
    l.Lb = n > 0 ? n : 0;
    return l;
}

// DIR +1: out[t] = sum_j w[j] in[t + j] (taps < Lb);   DIR -1: out[t] = sum_j w[j] in[t - j] (taps >= 0).   t < Lb, zeros past it.
template <int V, int DIR>
__global__ __launch_bounds__(LA_THREADS) void lookahead_conv_kernel(const float* __restrict__ in, const float* __restrict__ w,
                                                                    const int* __restrict__ lengths, int T, int B, int H, int context,
                                                                    int t_chunk, float* __restrict__ out) {
    typedef typename LaVec<V>::type vec;
    extern __shared__ __attribute__((aligned(16))) float la_lds[];
    const int R = context + LA_U;
    vec* ring = reinterpret_cast<vec*>(la_lds) + threadIdx.x;                             // [R][LA_THREADS]
    vec* wts = reinterpret_cast<vec*>(la_lds) + (long)R * LA_THREADS + threadIdx.x;       // [context + 1][LA_THREADS]
    const LaLane l = la_lane(lengths, T, B, H, V);
    if (!l.active) return;                                  // (no barrier below)
    const long frame = (long)B * H;
    const int t0 = blockIdx.y * t_chunk;
    const int t1 = t0 + t_chunk < T ? t0 + t_chunk : T;
    const int Lb = l.Lb;
    for (int j = 0; j <= context; ++j) wts[j * LA_THREADS] = *reinterpret_cast<const vec*>(w + (long)j * H + l.h);

    // the window of frame t covers the times base(t) .. base(t) + context; slot of time tau = (tau - base(t0)) mod R
    const int base0 = DIR > 0 ? t0 : t0 - context;
    // the `context` frames in front of the first block's own: times base0 .. base0 + context - 1, slots 0 .. context - 1
    for (int k0 = 0; k0 < context; k0 += LA_U) {
        vec v[LA_U];
#pragma unroll
        for (int u = 0; u < LA_U; ++u) {
            const int tau = base0 + k0 + u;
            v[u] = LaVec<V>::zero();
            if (k0 + u < context && tau >= 0 && tau < Lb) v[u] = *reinterpret_cast<const vec*>(in + (long)tau * frame + l.col);
        }
#pragma unroll
        for (int u = 0; u < LA_U; ++u)
            if (k0 + u < context) ring[(k0 + u) * LA_THREADS] = v[u];
    }
    int slot_new = context % R;                             // slot of the time that enters with frame tb: base(tb) + context
    int slot_t = DIR > 0 ? 0 : context % R;                 // slot of time tb itself
    const vec w0 = wts[0];
    for (int tb = t0; tb < t1; tb += LA_U) {
        vec v[LA_U];
#pragma unroll
        for (int u = 0; u < LA_U; ++u) {
            const int t = tb + u;
            const int tau = (DIR > 0 ? t : t - context) + context;
            v[u] = LaVec<V>::zero();
            if (t < t1 && tau < Lb) v[u] = *reinterpret_cast<const vec*>(in + (long)tau * frame + l.col);      // (tau >= t >= 0)
        }
        {
            int s = slot_new;
#pragma unroll
            for (int u = 0; u < LA_U; ++u) {
                ring[s * LA_THREADS] = v[u];
                s = s + 1 == R ? 0 : s + 1;
            }
            slot_new = s;
        }
        // LA_U outputs at once: per tap one weight and LA_U independent ring reads, LA_U independent fmaf chains.  The reads are
        // unconditional (every slot holds a frame or the zeros that stand for one outside the row); a tap outside the row is
        // computed and DROPPED by a select, never added -- and where a tap lies in the row for all of the wave, there is no select
        vec acc[LA_U];
        {
            int s = slot_t;
#pragma unroll
            for (int u = 0; u < LA_U; ++u) {
                acc[u] = LaVec<V>::mul(w0, ring[s * LA_THREADS]);
                s = s + 1 == R ? 0 : s + 1;
            }
        }
        int sj = slot_t;                                    // slot of the tap j of frame tb
        for (int j = 1; j <= context; ++j) {
            if (DIR > 0) sj = sj + 1 == R ? 0 : sj + 1;
            else sj = sj == 0 ? R - 1 : sj - 1;
            const vec wj = wts[j * LA_THREADS];
            const int room = DIR > 0 ? Lb - j - tb : tb - j;      // forward: tap j of frame tb + u lies in the row iff u < room; backward: iff u + room >= 0
            int s = sj;
            if (__all(DIR > 0 ? LA_U - 1 < room : room >= 0)) {      // (uniform) the tap lies in the row for the whole block, in every lane: no select
#pragma unroll
                for (int u = 0; u < LA_U; ++u) {
                    acc[u] = LaVec<V>::fma(wj, ring[s * LA_THREADS], acc[u]);
                    s = s + 1 == R ? 0 : s + 1;
                }
            } else {
#pragma unroll
                for (int u = 0; u < LA_U; ++u) {
                    const vec f = LaVec<V>::fma(wj, ring[s * LA_THREADS], acc[u]);
                    const bool in_row = DIR > 0 ? u < room : u + room >= 0;
                    acc[u] = in_row ? f : acc[u];
                    s = s + 1 == R ? 0 : s + 1;
                }
            }
        }
#pragma unroll
        for (int u = 0; u < LA_U; ++u) {
            const int t = tb + u;
            if (t < t1) *reinterpret_cast<vec*>(out + (long)t * frame + l.col) = t < Lb ? acc[u] : LaVec<V>::zero();
        }
        slot_t = (slot_t + LA_U) % R;
    }
}

// part[chunk][b][j][h] = sum_{t in the chunk, t + j < Lb} dy[t][b][h] * x[t + j][b][h],  ascending t, one fmaf chain per (j, lane).
template <int V>
__global__ __launch_bounds__(LA_THREADS) void lookahead_dw_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                                                  const int* __restrict__ lengths, int T, int B, int H, int context,
                                                                  int t_chunk, float* __restrict__ part) {
    typedef typename LaVec<V>::type vec;
    extern __shared__ __attribute__((aligned(16))) float la_lds[];
    const int R = context + LA_U;
    vec* ring = reinterpret_cast<vec*>(la_lds) + threadIdx.x;                             // [R][LA_THREADS]   frames of x
    vec* sums = reinterpret_cast<vec*>(la_lds) + (long)R * LA_THREADS + threadIdx.x;      // [context + 1][LA_THREADS]
    const LaLane l = la_lane(lengths, T, B, H, V);
    if (!l.active) return;
    const long frame = (long)B * H;
    const int t0 = blockIdx.y * t_chunk;
    const int t1 = t0 + t_chunk < T ? t0 + t_chunk : T;
    const int Lb = l.Lb;
    for (int j = 0; j <= context; ++j) sums[j * LA_THREADS] = LaVec<V>::zero();

    for (int k0 = 0; k0 < context; k0 += LA_U) {            // x[t0 .. t0 + context - 1] into slots 0 .. context - 1
        vec v[LA_U];
#pragma unroll
        for (int u = 0; u < LA_U; ++u) {
            const int tau = t0 + k0 + u;
            v[u] = LaVec<V>::zero();
            if (k0 + u < context && tau < Lb) v[u] = *reinterpret_cast<const vec*>(x + (long)tau * frame + l.col);
        }
#pragma unroll
        for (int u = 0; u < LA_U; ++u)
            if (k0 + u < context) ring[(k0 + u) * LA_THREADS] = v[u];
    }
    int slot_new = context % R, slot_t = 0;
    for (int tb = t0; tb < t1; tb += LA_U) {
        vec v[LA_U], g[LA_U];
#pragma unroll
        for (int u = 0; u < LA_U; ++u) {
            const int t = tb + u;
            v[u] = g[u] = LaVec<V>::zero();
            if (t < t1 && t + context < Lb) v[u] = *reinterpret_cast<const vec*>(x + (long)(t + context) * frame + l.col);
            if (t < t1 && t < Lb) g[u] = *reinterpret_cast<const vec*>(dy + (long)t * frame + l.col);
        }
        {
            int s = slot_new;
#pragma unroll
            for (int u = 0; u < LA_U; ++u) {
                ring[s * LA_THREADS] = v[u];
                s = s + 1 == R ? 0 : s + 1;
            }
            slot_new = s;
        }
        int sj = slot_t;                                    // slot of time tb + j
        for (int j = 0; j <= context; ++j) {
            vec acc = sums[j * LA_THREADS];
            int s = sj;
#pragma unroll
            for (int u = 0; u < LA_U; ++u) {
                // (unconditional: outside the row or the chunk g[u] is zero, and a slot past the row holds zeros -- the term is +0)
                acc = LaVec<V>::fma(g[u], ring[s * LA_THREADS], acc);
                s = s + 1 == R ? 0 : s + 1;
            }
            sums[j * LA_THREADS] = acc;
            sj = sj + 1 == R ? 0 : sj + 1;
        }
        slot_t = (slot_t + LA_U) % R;
    }
    float* tile = part + ((long)blockIdx.y * B + l.b) * (long)(context + 1) * H + l.h;
    for (int j = 0; j <= context; ++j) *reinterpret_cast<vec*>(tile + (long)j * H) = sums[j * LA_THREADS];
}

// dw[e] += sum_p part[p][e], e = j * H + h: slice s of LA_SLICES sums the partials [s * per_slice, (s + 1) * per_slice) in index
// order, the slices are added in slice order, then one add into dw.
__global__ __launch_bounds__(LA_SLICES * LA_RED_COLS) void lookahead_dw_reduce_kernel(const float* __restrict__ part, int n_part,
                                                                                       int per_slice, long n_elem,
                                                                                       float* __restrict__ dw) {
    __shared__ float red[LA_SLICES][LA_RED_COLS];
    const int c = threadIdx.x % LA_RED_COLS, s = threadIdx.x / LA_RED_COLS;
    const long e = (long)blockIdx.x * LA_RED_COLS + c;
    float acc = 0.f;
    if (e < n_elem) {
        const int p0 = s * per_slice;
        const int p1 = p0 + per_slice < n_part ? p0 + per_slice : n_part;
        for (int p = p0; p < p1; ++p) acc += part[(long)p * n_elem + e];
    }
    red[s][c] = acc;
    __syncthreads();
    if (s == 0 && e < n_elem) {
        float tot = red[0][c];
        for (int q = 1; q < LA_SLICES; ++q) tot += red[q][c];
        dw[e] += tot;
    }
}

// ---- the plan: the launch geometry as plain numbers (amdspeech.h: amdspeech_lookahead_plan_info).  The calls plan first and LAUNCH
// from the struct; amdspeech_lookahead_plan returns the same struct.  No device is needed.
static int plan_lookahead(int T, int B, int H, int context, bool aligned, LaPlan* p) {
    AS_CHECK_ARG(T > 0 && B > 0 && H > 0, "lookahead: bad shape (T %d, B %d, H %d)", T, B, H);
    AS_CHECK_ARG((long)B * H < (1L << 31) && (long)T * B < (1L << 31), "lookahead: shape too large (T %d, B %d, H %d)", T, B, H);
    AS_CHECK_ARG(context >= 1 && context <= LA_MAX_CONTEXT, "lookahead: context %d outside 1 .. %d", context, LA_MAX_CONTEXT);
    p->vec = (H % 4 == 0 && aligned) ? 4 : 1;
    p->unroll = LA_U;
    p->col_blocks = ceil_div((long)B * H / p->vec, LA_THREADS);
    // enough chunks that the grid covers the chip, but none so short that its halo of `context` frames weighs more than a quarter
    int tc = ceil_div(T, ceil_div(LA_TARGET_WGS, p->col_blocks));
    const int floor_tc = LA_HALO_FACTOR * context;
    tc = tc > floor_tc ? tc : floor_tc;
    p->t_chunk = ceil_div(tc, LA_U) * LA_U;                 // whole blocks
    p->chunks = ceil_div(T, p->t_chunk);
    const long wgs = (long)p->col_blocks * p->chunks;
    AS_CHECK_ARG(p->chunks <= 65535 && wgs < (1L << 31), "lookahead: T %d, B %d, H %d would take %ld workgroups", T, B, H, wgs);
    p->workgroups = (int)wgs;
    p->lds_bytes = (context + LA_U + context + 1) * LA_THREADS * p->vec * (int)sizeof(float);
    p->dw_partials = p->chunks * B;
    p->dw_terms = p->t_chunk;
    p->reduce_slices = LA_SLICES;
    p->reduce_terms = ceil_div(p->dw_partials, LA_SLICES);
    p->reduce_workgroups = ceil_div((long)(context + 1) * H, LA_RED_COLS);
    return AMDSPEECH_OK;
}

// Bytes of the partial tiles for this shape AND every shorter T (a caller sizes it once for its padded length and runs prefixes):
// chunks never exceed ceil(1024 / col_blocks), nor ceil(T / the chunk floor), and both bounds grow with T.
static size_t lookahead_ws_bytes(const LaPlan& p, int T, int B, int H, int context) {
    const int by_grid = ceil_div(LA_TARGET_WGS, p.col_blocks);
    const int by_floor = ceil_div(T, ceil_div(LA_HALO_FACTOR * context, LA_U) * LA_U);
    const int most = by_grid < by_floor ? by_grid : by_floor;
    return (size_t)most * B * (size_t)(context + 1) * (size_t)H * sizeof(float);
}

static bool la_overlap(const void* a, const void* b, size_t bytes) {
    const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
    return !(x + bytes <= y || y + bytes <= x);
}

static bool la_aligned(std::initializer_list<const void*> ptrs) {
    uintptr_t any = 0;
    for (const void* q : ptrs) any |= reinterpret_cast<uintptr_t>(q);
    return (any & 15) == 0;
}

// The two V = 4 walks may take more dynamic LDS than a kernel gets unasked (context 32: 73 KiB).
template <typename K>
static int la_allow_lds(K kernel, unsigned long long* seen) {
    if (DeviceOnce once{seen}) {
        const int most = (2 * LA_MAX_CONTEXT + LA_U + 1) * LA_THREADS * 4 * (int)sizeof(float);
        AS_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, most));
        once.done();
    }
    return AMDSPEECH_OK;
}

template <int DIR>
static int launch_conv(hipStream_t s, const LaPlan& pl, const float* in, const float* w, const int* lengths, int T, int B, int H,
                       int context, float* out) {
    const dim3 grid(pl.col_blocks, pl.chunks), block(LA_THREADS);
    if (pl.vec == 4) {
        static unsigned long long seen = 0;
        if (int rc = la_allow_lds(lookahead_conv_kernel<4, DIR>, &seen)) return rc;
        hipLaunchKernelGGL((lookahead_conv_kernel<4, DIR>), grid, block, pl.lds_bytes, s, in, w, lengths, T, B, H, context, pl.t_chunk, out);
    } else {
        hipLaunchKernelGGL((lookahead_conv_kernel<1, DIR>), grid, block, pl.lds_bytes, s, in, w, lengths, T, B, H, context, pl.t_chunk, out);
    }
    AS_CHECK_LAUNCH();
    return AMDSPEECH_OK;
}

static int run_lookahead_fwd(hipStream_t s, const float* x, const float* w, const int* lengths, int T, int B, int H, int context,
                             float* y) {
    AS_CHECK_ARG(x && w && lengths && y, "lookahead_fwd: null pointer");
    LaPlan pl;
    if (int rc = plan_lookahead(T, B, H, context, la_aligned({x, w, y}), &pl)) return rc;
    AS_CHECK_ARG(!la_overlap(x, y, (size_t)T * B * H * sizeof(float)), "lookahead_fwd: x and y overlap");
    return launch_conv<+1>(s, pl, x, w, lengths, T, B, H, context, y);
}

static int run_lookahead_bwd(hipStream_t s, const float* x, const float* w, const float* dy, const int* lengths, int T, int B, int H,
                             int context, float* dx, float* dw, void* ws) {
    AS_CHECK_ARG(x && w && dy && lengths && dx && dw && ws, "lookahead_bwd: null pointer");
    LaPlan pl;
    if (int rc = plan_lookahead(T, B, H, context, la_aligned({x, w, dy, dx, ws}), &pl)) return rc;
    const size_t bytes = (size_t)T * B * H * sizeof(float);
    AS_CHECK_ARG(!la_overlap(dy, dx, bytes), "lookahead_bwd: dy and dx overlap");
    AS_CHECK_ARG(!la_overlap(x, dx, bytes), "lookahead_bwd: x and dx overlap");
    AS_CHECK_ARG((reinterpret_cast<uintptr_t>(ws) & 3) == 0, "lookahead_bwd: the workspace must be 4-byte aligned");
    if (int rc = launch_conv<-1>(s, pl, dy, w, lengths, T, B, H, context, dx)) return rc;
    const dim3 grid(pl.col_blocks, pl.chunks), block(LA_THREADS);
    float* part = static_cast<float*>(ws);
    if (pl.vec == 4) {
        static unsigned long long seen = 0;
        if (int rc = la_allow_lds(lookahead_dw_kernel<4>, &seen)) return rc;
        hipLaunchKernelGGL((lookahead_dw_kernel<4>), grid, block, pl.lds_bytes, s, x, dy, lengths, T, B, H, context, pl.t_chunk, part);
    } else {
        hipLaunchKernelGGL((lookahead_dw_kernel<1>), grid, block, pl.lds_bytes, s, x, dy, lengths, T, B, H, context, pl.t_chunk, part);
    }
    AS_CHECK_LAUNCH();
    hipLaunchKernelGGL(lookahead_dw_reduce_kernel, dim3(pl.reduce_workgroups), dim3(LA_SLICES * LA_RED_COLS), 0, s, part, pl.dw_partials,
                       pl.reduce_terms, (long)(context + 1) * H, dw);
    AS_CHECK_LAUNCH();
    return AMDSPEECH_OK;
}

}  // namespace amdspeech

using namespace amdspeech;

extern "C" int amdspeech_lookahead_plan(int T, int B, int H, int context, amdspeech_lookahead_plan_info* out) {
    AS_CHECK_ARG(out != nullptr, "lookahead_plan: null output");
    return plan_lookahead(T, B, H, context, true, out);
}

extern "C" size_t amdspeech_lookahead_bwd_workspace_bytes(int T, int B, int H, int context) {
    LaPlan pl;
    if (plan_lookahead(T, B, H, context, true, &pl) != AMDSPEECH_OK) return 0;
    return lookahead_ws_bytes(pl, T, B, H, context);
}

extern "C" int amdspeech_lookahead_fwd(void* stream, const float* x, const float* w, const int* lengths, int T, int B, int H,
                                       int context, float* y) {
    return run_lookahead_fwd(static_cast<hipStream_t>(stream), x, w, lengths, T, B, H, context, y);
}

extern "C" int amdspeech_lookahead_bwd(void* stream, const float* x, const float* w, const float* dy, const int* lengths, int T, int B,
                                       int H, int context, float* dx, float* dw, void* ws) {
    return run_lookahead_bwd(static_cast<hipStream_t>(stream), x, w, dy, lengths, T, B, H, context, dx, dw, ws);
}
