// Feature normalisation between the front end and frame stacking: per-utterance or global cepstral mean and variance normalisation,
// IN PLACE on the front end's [t_in][B][D] tensor (amdspeech.h: amdspeech_feature_norm, amdspeech_feature_moments).  No reference
// counterpart (an opt-in deviation).  The input needs no gradient, so there is no backward kernel.
//
//   n = min(n_b, t_in);  mean = (1/n) sum_{t<n} x[t][b][d];  var = (1/n) sum_{t<n} (x[t][b][d] - mean)^2      (population variance)
//   x[t][b][d] = float((double(x[t][b][d]) - mean) * scale)   for t < n,    scale = norm_vars ? 1 / sqrt(max(var, var_floor)) : 1
//
// Two launches in utterance mode, one in global mode; grid (split, rows), 256 threads; workgroup (s, b) owns time slice s of row b.
//   feature_moments_kernel   float64 sums of the slice, SHIFTED by the row's own first frame K[d] = x[0][b][d]: S' = sum (x - K),
//                            Q' = sum (x - K)^2.  The shift is the same in every slice of a row, so the slices' partials add
//                            directly; it makes a constant dim exactly zero-variance and keeps the single pass accurate when
//                            |mean| >> std (c0 of an MFCC sits near -1131).  One [2][D] partial per (b, s) and the row's K (slice 0
//                            writes it: the apply kernel overwrites frame 0 while other slices still need K) go to the workspace.
//   feature_norm_apply_kernel  sums the row's partials in slice order, forms mean = K + S'/n, var = max(Q'/n - (S'/n)^2, 0) and
//                            scale in float64 once per workgroup into LDS (global mode: copies the table instead), then re-reads the
//                            slice's frames (5 MB at the headline shape: L2 / Infinity Cache) and stores them normalised.
//   feature_moments_finish_kernel  (amdspeech_feature_moments only) mean and M2 = Q' - S'^2 / n per row, for the corpus statistics.
// Threads are (frame slot, vector column): `lanes` = the smallest power of two that covers the D / V vector columns (at most 256)
// share a frame, 256 / lanes frame slots stride over the slice's frames; columns beyond 256 lanes are looped, so both kernels keep a
// fixed 4096 V bytes of static LDS whatever D (no dynamic LDS, no attribute call).  V = 4: 16-byte loads and stores.
// No atomics: the slots' partials meet in LDS and are summed in slot order, the slices' in slice order -- two runs give the same
// bits.  Frames at or past n are neither read nor written; a row with n = 0 is not touched.
#include "row_args.h"

#include <cmath>


namespace amdspeech {

constexpr int FN_THREADS = 256;
constexpr int FN_MAX_WGS = 2048;          // cap of the grid, as the sibling kernels cap theirs; rows beyond it are strided
constexpr int FN_TARGET_WGS = 512;        // two workgroups per CU: what `split` aims for when the rows alone are fewer
constexpr int FN_MIN_PASSES = 4;          // a slice is no shorter than this many frame-slot passes
constexpr int FN_MAX_WIDTH = 4096;        // D (frame_stack.hip: FS_MAX_WIDTH)

typedef amdspeech_feature_norm_plan_info FnPlan;
typedef amdspeech_feature_norm_desc FnDesc;

static __host__ __device__ inline int fn_lanes(int cols) {
    int l = 1;
    while (l < cols && l < FN_THREADS) l *= 2;
    return l;
}

// Words of the workspace per row: `split` partials [2][D] and the row's shift K [D], all float64.
static __host__ __device__ inline long fn_row_doubles(int split, int D) { return (2L * split + 1) * D; }

template <int V>
static __device__ inline void fn_load(const float* p, float (&v)[V]) {
    if constexpr (V == 4) {
        const f32x4 q = *reinterpret_cast<const f32x4*>(p);
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else {
        v[0] = *p;
    }
}

template <int V, bool LEN_ARG>
__global__ __launch_bounds__(FN_THREADS) void feature_moments_kernel(const float* __restrict__ x, RowArgs len_arg,
                                                                     const int* __restrict__ len_dev, int B, int D, int t_in, int slice,
                                                                     int lanes, double* __restrict__ ws) {
    __shared__ double red[FN_THREADS * 2 * V];             // [slot][lane][S' x V, Q' x V]
    const int cols = D / V, slots = FN_THREADS / lanes;
    const int slot = threadIdx.x / lanes, lane = threadIdx.x - slot * lanes;
    const int s = blockIdx.x, split = gridDim.x;
    for (int b = blockIdx.y; b < B; b += gridDim.y) {
        int n = row_arg<LEN_ARG>(len_arg, len_dev, b);
        n = n < t_in ? n : t_in;                           // (the front end's counts are not clipped to its t_max)
        const int t0 = s * slice;
        int t1 = t0 + slice;
        t1 = t1 < n ? t1 : n;                              // frames at or past n are never read
        double* row = ws + (long)b * fn_row_doubles(split, D);
        double* part = row + (long)s * 2 * D;
        for (int c0 = 0; c0 < cols; c0 += lanes) {
            const int c = c0 + lane;
            double S[V], Q[V];
            for (int i = 0; i < V; ++i) S[i] = Q[i] = 0.0;
            if (c < cols && n > 0) {
                float k[V];
                fn_load<V>(x + (long)b * D + (long)c * V, k);              // frame 0 of the row
                if (s == 0 && slot == 0)
                    for (int i = 0; i < V; ++i) row[2L * split * D + (long)c * V + i] = (double)k[i];
                for (int t = t0 + slot; t < t1; t += slots) {
                    float v[V];
                    fn_load<V>(x + ((long)t * B + b) * D + (long)c * V, v);
                    for (int i = 0; i < V; ++i) {
                        const double d = (double)v[i] - (double)k[i];
                        S[i] += d;
                        Q[i] += d * d;
                    }
                }
            } else if (c < cols && s == 0 && slot == 0) {
                for (int i = 0; i < V; ++i) row[2L * split * D + (long)c * V + i] = 0.0;
            }
            double* mine = red + (long)threadIdx.x * 2 * V;
            for (int i = 0; i < V; ++i) {
                mine[i] = S[i];
                mine[V + i] = Q[i];
            }
            __syncthreads();
            // the slots' partials, summed in slot order: work item w = (lane, one of the 2 V sums)
            for (int w = threadIdx.x; w < lanes * 2 * V; w += FN_THREADS) {
                const int l = w / (2 * V), j = w - l * (2 * V);
                if (c0 + l >= cols) continue;
                double acc = 0.0;
                for (int q = 0; q < slots; ++q) acc += red[((long)q * lanes + l) * 2 * V + j];
                const int which = j / V, i = j - which * V;
                part[(long)which * D + (long)(c0 + l) * V + i] = acc;
            }
            __syncthreads();
        }
    }
}

template <int V, bool GLOBAL, bool LEN_ARG>
__global__ __launch_bounds__(FN_THREADS) void feature_norm_apply_kernel(float* __restrict__ x, RowArgs len_arg,
                                                                        const int* __restrict__ len_dev, int B, int D, int t_in,
                                                                        int slice, int lanes, const double* __restrict__ src,
                                                                        int norm_vars, double var_floor) {
    __shared__ double stat[FN_THREADS * 2 * V];            // [dim of this column pass][mean, scale]
    const int cols = D / V, slots = FN_THREADS / lanes;
    const int slot = threadIdx.x / lanes, lane = threadIdx.x - slot * lanes;
    const int s = blockIdx.x, split = gridDim.x;
    for (int b = blockIdx.y; b < B; b += gridDim.y) {
        int n = row_arg<LEN_ARG>(len_arg, len_dev, b);
        n = n < t_in ? n : t_in;
        const int t0 = s * slice;
        int t1 = t0 + slice;
        t1 = t1 < n ? t1 : n;
        if (t0 >= t1) continue;                            // (uniform in the workgroup) nothing of this row lies in the slice
        const double* row = src + (long)b * fn_row_doubles(split, D);
        for (int c0 = 0; c0 < cols; c0 += lanes) {
            const int d0 = c0 * V;
            int nd = lanes * V;
            nd = nd < D - d0 ? nd : D - d0;
            for (int i = threadIdx.x; i < nd; i += FN_THREADS) {
                double mean, scale;
                if (GLOBAL) {
                    mean = src[d0 + i];
                    scale = src[D + d0 + i];
                } else {
                    double S = 0.0, Q = 0.0;
                    for (int q = 0; q < split; ++q) {      // the slices' partials, in slice order
                        S += row[(long)q * 2 * D + d0 + i];
                        Q += row[(long)q * 2 * D + D + d0 + i];
                    }
                    const double m = S / (double)n;
                    mean = row[2L * split * D + d0 + i] + m;
                    double var = Q / (double)n - m * m;
                    var = var > 0.0 ? var : 0.0;
                    scale = norm_vars ? 1.0 / sqrt(var > var_floor ? var : var_floor) : 1.0;
                }
                stat[2 * i] = mean;
                stat[2 * i + 1] = scale;
            }
            __syncthreads();
            const int c = c0 + lane;
            if (c < cols) {
                double mean[V], scale[V];
                for (int i = 0; i < V; ++i) {
                    mean[i] = stat[2 * (lane * V + i)];
                    scale[i] = stat[2 * (lane * V + i) + 1];
                }
                for (int t = t0 + slot; t < t1; t += slots) {
                    float* p = x + ((long)t * B + b) * D + (long)c * V;
                    float v[V];
                    fn_load<V>(p, v);
                    for (int i = 0; i < V; ++i) v[i] = (float)(((double)v[i] - mean[i]) * scale[i]);      // rounded once
                    if constexpr (V == 4) {
                        const f32x4 q = {v[0], v[1], v[2], v[3]};
                        *reinterpret_cast<f32x4*>(p) = q;
                    } else {
                        *p = v[0];
                    }
                }
            }
            __syncthreads();
        }
    }
}

// moments[b] = [mean[D], M2[D]],  M2 = sum (x - mean)^2 = Q' - S'^2 / n;  zeros for n = 0.  One thread per (row, dim).
template <bool LEN_ARG>
__global__ __launch_bounds__(FN_THREADS) void feature_moments_finish_kernel(const double* __restrict__ ws, RowArgs len_arg,
                                                                            const int* __restrict__ len_dev, int B, int D, int t_in,
                                                                            int split, double* __restrict__ moments) {
    const long total = (long)B * D;
    for (long e = (long)blockIdx.x * FN_THREADS + threadIdx.x; e < total; e += (long)gridDim.x * FN_THREADS) {
        const int b = (int)(e / D), d = (int)(e - (long)b * D);
        int n = row_arg<LEN_ARG>(len_arg, len_dev, b);
        n = n < t_in ? n : t_in;
        double mean = 0.0, m2 = 0.0;
        if (n > 0) {
            const double* row = ws + (long)b * fn_row_doubles(split, D);
            double S = 0.0, Q = 0.0;
            for (int q = 0; q < split; ++q) {
                S += row[(long)q * 2 * D + d];
                Q += row[(long)q * 2 * D + D + d];
            }
            mean = row[2L * split * D + d] + S / (double)n;
            m2 = Q - S * (S / (double)n);
            m2 = m2 > 0.0 ? m2 : 0.0;
        }
        moments[(long)b * 2 * D + d] = mean;
        moments[(long)b * 2 * D + D + d] = m2;
    }
}

// ---- the plan: the launch geometry as plain numbers (amdspeech.h: amdspeech_feature_norm_plan_info).  Both calls plan first and
// LAUNCH from the struct; amdspeech_feature_norm_plan returns the same struct.  No device is needed.
static int plan_feature_norm(int B, int D, int t_in, int mode, FnPlan* p) {
    AS_CHECK_ARG(B > 0 && D > 0 && t_in > 0 && (long)t_in * B < (1L << 31), "feature_norm: bad shape (B %d, D %d, t_in %d)", B, D, t_in);
    AS_CHECK_ARG(D <= FN_MAX_WIDTH, "feature_norm: D = %d exceeds %d", D, FN_MAX_WIDTH);
    AS_CHECK_ARG(mode >= AMDSPEECH_FEATURE_NORM_NONE && mode <= AMDSPEECH_FEATURE_NORM_GLOBAL, "feature_norm: mode %d is none of 0 (none), 1 (utterance), 2 (global)", mode);
    p->vec = D % 4 == 0 ? 4 : 1;
    const int slots = FN_THREADS / fn_lanes(D / p->vec);
    const int rows = B < FN_MAX_WGS ? B : FN_MAX_WGS;
    int split = ceil_div(FN_TARGET_WGS, rows);                      // so that a small batch still covers the chip ...
    const int by_length = t_in / (FN_MIN_PASSES * slots);           // ... in slices of at least FN_MIN_PASSES passes
    split = split < by_length ? split : by_length;
    split = split < 1 ? 1 : split;
    const int slice = ceil_div(t_in, split);
    p->split = ceil_div(t_in, slice);                               // (no empty slice)
    p->workgroups = mode == AMDSPEECH_FEATURE_NORM_NONE ? 0 : p->split * rows;
    p->lds_bytes = FN_THREADS * 2 * p->vec * (int)sizeof(double);
    p->meta_by_copy = B > ROW_ARGS_MAX ? 1 : 0;
    const long bytes = mode == AMDSPEECH_FEATURE_NORM_UTTERANCE ? (long)B * fn_row_doubles(p->split, D) * (long)sizeof(double) : 0;
    AS_CHECK_ARG(bytes < (1L << 31), "feature_norm: the workspace of B %d, D %d would take %ld bytes", B, D, bytes);
    p->workspace_bytes = (int)bytes;
    return AMDSPEECH_OK;
}

static int check_lengths(const int* n_frames, int B) {
    for (int b = 0; b < B; ++b)
        AS_CHECK_ARG(n_frames[b] >= 0, "feature_norm: n_frames[%d] = %d is negative", b, n_frames[b]);
    return AMDSPEECH_OK;
}

// What a call launches: 0 the moments and the apply kernel (utterance mode), 1 the apply kernel from a table (global mode),
// 2 the moments and the finish kernel (amdspeech_feature_moments).
enum { FN_UTTERANCE = 0, FN_GLOBAL = 1, FN_MOMENTS = 2 };

template <int V, bool LEN_ARG>
static hipError_t launch_feature_norm(hipStream_t s, int what, const FnPlan& pl, float* x, const RowArgs& la, const int* d_len, int B, int D,
                                      int t_in, const FnDesc* desc, const double* table, double* ws, double* moments) {
    const int rows = B < FN_MAX_WGS ? B : FN_MAX_WGS;
    const dim3 grid(pl.split, rows), block(FN_THREADS);
    const int slice = ceil_div(t_in, pl.split), lanes = fn_lanes(D / V);
    if (what != FN_GLOBAL)
        hipLaunchKernelGGL((feature_moments_kernel<V, LEN_ARG>), grid, block, 0, s, x, la, d_len, B, D, t_in, slice, lanes, ws);
    if (what == FN_UTTERANCE)
        hipLaunchKernelGGL((feature_norm_apply_kernel<V, false, LEN_ARG>), grid, block, 0, s, x, la, d_len, B, D, t_in, slice, lanes, ws,
                           desc->norm_vars, desc->var_floor);
    else if (what == FN_GLOBAL)
        hipLaunchKernelGGL((feature_norm_apply_kernel<V, true, LEN_ARG>), grid, block, 0, s, x, la, d_len, B, D, t_in, slice, lanes, table,
                           desc->norm_vars, desc->var_floor);
    else {
        const long wgs = ((long)B * D + FN_THREADS - 1) / FN_THREADS;
        hipLaunchKernelGGL((feature_moments_finish_kernel<LEN_ARG>), dim3((unsigned)(wgs < FN_MAX_WGS ? wgs : FN_MAX_WGS)), block, 0, s, ws,
                           la, d_len, B, D, t_in, pl.split, moments);
    }
    return hipGetLastError();
}

static int run_feature_norm(hipStream_t s, int what, float* x, const int* n_frames, int B, int D, int t_in, const FnDesc* desc,
                            const double* table, double* ws, double* moments) {
    AS_CHECK_ARG(x && n_frames, "feature_norm: null pointer");
    FnPlan pl;
    const int mode = what == FN_GLOBAL ? AMDSPEECH_FEATURE_NORM_GLOBAL : AMDSPEECH_FEATURE_NORM_UTTERANCE;
    if (int rc = plan_feature_norm(B, D, t_in, mode, &pl)) return rc;
    AS_CHECK_ARG(what == FN_GLOBAL ? table != nullptr : ws != nullptr, "feature_norm: null %s", what == FN_GLOBAL ? "table" : "workspace");
    AS_CHECK_ARG(what != FN_MOMENTS || moments != nullptr, "feature_norm: null moments");
    AS_CHECK_ARG(pl.vec == 1 || (reinterpret_cast<uintptr_t>(x) & 15) == 0, "feature_norm: x must be 16-byte aligned when D is a multiple of 4");
    AS_CHECK_ARG(((reinterpret_cast<uintptr_t>(ws) | reinterpret_cast<uintptr_t>(table) | reinterpret_cast<uintptr_t>(moments)) & 7) == 0,
                 "feature_norm: the float64 buffers must be 8-byte aligned");
    if (int rc = check_lengths(n_frames, B)) return rc;

    // (more rows than the argument block holds: with_row_args waits for the kernels, as frame_stack.hip's call does)
    return with_row_args(s, n_frames, B, [&](auto by_arg, const RowArgs& la, const int* d_len) {
        constexpr bool LEN_ARG = decltype(by_arg)::value;
        return pl.vec == 4 ? launch_feature_norm<4, LEN_ARG>(s, what, pl, x, la, d_len, B, D, t_in, desc, table, ws, moments)
                           : launch_feature_norm<1, LEN_ARG>(s, what, pl, x, la, d_len, B, D, t_in, desc, table, ws, moments);
    });
}

}  // namespace amdspeech

using namespace amdspeech;

extern "C" int amdspeech_feature_norm_plan(int B, int D, int t_in, int mode, amdspeech_feature_norm_plan_info* out) {
    AS_CHECK_ARG(out != nullptr, "feature_norm_plan: null output");
    return plan_feature_norm(B, D, t_in, mode, out);
}

extern "C" int amdspeech_feature_moments(void* stream, const float* x, const int* n_frames, int B, int D, int t_in, void* workspace,
                                         double* moments) {
    return run_feature_norm(static_cast<hipStream_t>(stream), FN_MOMENTS, const_cast<float*>(x), n_frames, B, D, t_in, nullptr, nullptr,
                            static_cast<double*>(workspace), moments);
}

extern "C" int amdspeech_feature_norm(void* stream, float* x, const int* n_frames, int B, int D, int t_in,
                                      const amdspeech_feature_norm_desc* desc, const double* table, void* workspace) {
    AS_CHECK_ARG(desc != nullptr, "feature_norm: null descriptor");
    AS_CHECK_ARG(desc->mode >= AMDSPEECH_FEATURE_NORM_NONE && desc->mode <= AMDSPEECH_FEATURE_NORM_GLOBAL,
                 "feature_norm: mode %d is none of 0 (none), 1 (utterance), 2 (global)", desc->mode);
    AS_CHECK_ARG(desc->var_floor > 0.0 && std::isfinite(desc->var_floor), "feature_norm: var_floor %g must be positive and finite", desc->var_floor);
    if (desc->mode == AMDSPEECH_FEATURE_NORM_NONE) {                // nothing is launched; the arguments are still checked
        FnPlan pl;
        AS_CHECK_ARG(x && n_frames, "feature_norm: null pointer");
        return plan_feature_norm(B, D, t_in, desc->mode, &pl);
    }
    const bool global = desc->mode == AMDSPEECH_FEATURE_NORM_GLOBAL;
    return run_feature_norm(static_cast<hipStream_t>(stream), global ? FN_GLOBAL : FN_UTTERANCE, x, n_frames, B, D, t_in, desc,
                            global ? table : nullptr, global ? nullptr : static_cast<double*>(workspace), nullptr);
}
