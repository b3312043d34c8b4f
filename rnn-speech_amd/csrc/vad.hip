// Voice activity over raw PCM and the ragged gather behind it: what cuts a long recording at its pauses into rows the model was
// trained on (amdspeech.h: amdspeech_vad_energy, amdspeech_vad_flags, amdspeech_gather_spans; host side: segmenter.py).  No
// reference counterpart (an opt-in deviation).  Plain launches only: no kernel waits for another workgroup.
//
//   vad_energy_kernel   grid (tiles of 63 frames, rows), 256 threads = 16 teams of 16 lanes.  A team owns one block of `hop` samples
//                       at a time: every lane sums the squares of its samples in float64 (lane l takes vectors l, l + 16, ... of
//                       four samples, or single samples l, l + 16, ... on the scalar path), the 16 partials meet in an xor
//                       butterfly (8, 4, 2, 1) -- a fixed order, two runs give the same bits.  64 block sums per tile land in LDS (the
//                       last one belongs to the next tile's first frame: 1 / 63 of the samples is read twice), then 63 threads form
//                       mean = (S[t] + S[t + 1]) / (2 hop) and the decibels.  The square of a float is exact in float64, so
//                       whether the compiler contracts x * x + acc into an FMA changes nothing.
//   vad_select_kernel   one workgroup of 1024 threads per row: the exact k-th smallest energy by a radix select over the order-
//                       preserving uint32 image of the floats, four 8-bit passes, 256 counters in LDS (integer LDS atomics; a thread
//                       adds a run of equal digits at once, since in the first passes nearly all keys share a digit), and the
//                       maximum; then the threshold in single float32 operations.
//   vad_flags_kernel    one workgroup of 1024 threads per row, every thread a contiguous chunk of the row.  With pz[t] the last frame
//                       <= t whose raw flag is 0, frame t is at least the min_run-th of its run iff raw[t] && t - pz[t] >= min_run
//                       (call that C[t]).  A run of min_run or more frames [a, b) has C set on [a + min_run - 1, b), so it meets the
//                       window [t - hangover, t + hangover] iff the LAST C at or before min(t + hangover + min_run - 1, F - 1) is
//                       >= t - hangover: opening and hangover together are two forward max-scans (pz, then the last C) and one
//                       lookup per frame.  The scans are chunk-local with an exclusive scan of the 1024 chunk results in LDS.
//   gather_spans_kernel every thread one 16-byte store of the flat [S * w_out] output; a 16-byte load where the four words lie
//                       in one span and their source is 16-byte aligned, single loads otherwise, zeros past the span.
#include "row_args.h"

#include <cmath>
#include <cstdlib>

namespace amdspeech {

constexpr int VAD_THREADS = 256;
constexpr int VAD_TEAM = 16;                                        // lanes that share one block sum
constexpr int VAD_TEAMS = VAD_THREADS / VAD_TEAM;
constexpr int VAD_TILE_BLOCKS = 4 * VAD_TEAMS;                      // block sums per workgroup: four rounds of the 16 teams
constexpr int VAD_TILE_FRAMES = VAD_TILE_BLOCKS - 1;                // a frame covers two blocks
constexpr int VAD_ROW_THREADS = 1024;                               // select and flags kernels: one workgroup per row
constexpr int VAD_SELECT_PASSES = 4;
constexpr int VAD_UNROLL = 8;                                       // frames whose loads a row-kernel thread issues together
constexpr int VAD_GRID_ROWS = 65535;                                // rows beyond the grid's y (or x) extent are strided
constexpr int VAD_MAX_HANGOVER = 1024;
constexpr float VAD_SILENCE_DB = -120.0f;                           // 10 log10(1e-12)
constexpr int GS_THREADS = 256;
constexpr int GS_ARGS_MAX = 256;                                    // spans that travel as kernel arguments

typedef amdspeech_vad_plan_info VadPlan;

template <bool VEC, bool LEN_ARG>
__global__ __launch_bounds__(VAD_THREADS) void vad_energy_kernel(const float* __restrict__ pcm, RowArgs len_arg,
                                                                 const int* __restrict__ len_dev, int B, int n_max, int hop,
                                                                 float* __restrict__ energy, int f_max) {
    __shared__ double S[VAD_TILE_BLOCKS];
    const int team = threadIdx.x / VAD_TEAM, lane = threadIdx.x - team * VAD_TEAM;
    const long t0 = (long)blockIdx.x * VAD_TILE_FRAMES;
    for (int b = blockIdx.y; b < B; b += gridDim.y) {
        int n = row_arg<LEN_ARG>(len_arg, len_dev, b);
        n = n < n_max ? n : n_max;
        const long F = ((long)n + hop - 1) / hop;
        const float* row = pcm + (long)b * n_max;
        for (int j = team; j < VAD_TILE_BLOCKS; j += VAD_TEAMS) {   // (the same four rounds for every team)
            const long t = t0 + j;
            double acc = 0.0;
            if (t < F) {                                            // block t holds a sample; S[F] and beyond stay 0
                const long lo = t * hop;
                const long end = lo + hop < n ? lo + hop : n;       // samples at or past n are never read
                const int len = (int)(end - lo);
                const float* p = row + lo;
                if constexpr (VEC) {
                    const int nv = len / 4;
                    for (int v = lane; v < nv; v += VAD_TEAM) {
                        const f32x4 q = *reinterpret_cast<const f32x4*>(p + 4 * v);
                        acc += (double)q.x * (double)q.x;
                        acc += (double)q.y * (double)q.y;
                        acc += (double)q.z * (double)q.z;
                        acc += (double)q.w * (double)q.w;
                    }
                    const int i = 4 * nv + lane;                    // the ragged end's last one to three samples
                    if (i < len) acc += (double)p[i] * (double)p[i];
                } else {
                    for (int i = lane; i < len; i += VAD_TEAM) acc += (double)p[i] * (double)p[i];
                }
            }
            for (int off = VAD_TEAM / 2; off > 0; off >>= 1) acc += __shfl_xor(acc, off, VAD_TEAM);
            if (lane == 0) S[j] = acc;
        }
        __syncthreads();
        const long t = t0 + threadIdx.x;
        if (threadIdx.x < VAD_TILE_FRAMES && t < f_max) {
            float e = VAD_SILENCE_DB;
            if (t < F) {
                const double mean = (S[threadIdx.x] + S[threadIdx.x + 1]) / (2.0 * (double)hop);
                if (isfinite(mean)) e = (float)(10.0 * log10(mean > 1e-12 ? mean : 1e-12));
            }
            energy[(long)b * f_max + t] = e;
        }
        __syncthreads();
    }
}

// float -> uint32 whose unsigned order is the floats' order (negative values reversed below the positive ones), and back
static __device__ __forceinline__ unsigned vad_key(float e) {
    const unsigned u = __float_as_uint(e);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
static __device__ __forceinline__ float vad_unkey(unsigned k) {
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

template <bool LEN_ARG>
__global__ __launch_bounds__(VAD_ROW_THREADS) void vad_select_kernel(const float* __restrict__ energy, RowArgs len_arg,
                                                                     const int* __restrict__ len_dev, int B, int f_max, int percentile,
                                                                     float margin_db, float range_db, float* __restrict__ stats) {
    __shared__ unsigned hist[256];
    __shared__ unsigned sel[2];                                     // the digits chosen so far, the rank inside them
    __shared__ unsigned peak_key;
    const int tid = threadIdx.x;
    for (int b = blockIdx.x; b < B; b += gridDim.x) {
        int F = row_arg<LEN_ARG>(len_arg, len_dev, b);
        F = F < f_max ? F : f_max;
        if (F <= 0) {                                               // (uniform in the workgroup)
            if (tid < 3) stats[3L * b + tid] = VAD_SILENCE_DB;
            continue;
        }
        const float* e = energy + (long)b * f_max;
        unsigned k = (unsigned)(((long)(F - 1) * percentile) / 100);
        unsigned prefix = 0;
        if (tid == 0) peak_key = 0;
        for (int pass = 0; pass < VAD_SELECT_PASSES; ++pass) {
            const int shift = 24 - 8 * pass;
            if (tid < 256) hist[tid] = 0;
            __syncthreads();
            unsigned mx = 0, cur = 0, cnt = 0;
            for (int t0 = tid; t0 < F; t0 += VAD_UNROLL * VAD_ROW_THREADS) {
                unsigned key[VAD_UNROLL];                           // the loads of a step are issued together: one workgroup has to
#pragma unroll                                                      // hide the memory latency by itself
                for (int j = 0; j < VAD_UNROLL; ++j) {
                    const int t = t0 + j * VAD_ROW_THREADS;
                    key[j] = vad_key(e[t < F ? t : F - 1]);
                }
#pragma unroll
                for (int j = 0; j < VAD_UNROLL; ++j) {
                    if (t0 + j * VAD_ROW_THREADS >= F) break;
                    if (pass == 0) mx = mx > key[j] ? mx : key[j];
                    if (pass == 0 || (key[j] >> (shift + 8)) == prefix) {
                        const unsigned bin = (key[j] >> shift) & 255u;
                        if (cnt && bin != cur) {
                            atomicAdd(&hist[cur], cnt);
                            cnt = 0;
                        }
                        cur = bin;
                        ++cnt;
                    }
                }
            }
            if (cnt) atomicAdd(&hist[cur], cnt);
            if (pass == 0) atomicMax(&peak_key, mx);
            __syncthreads();
            if (tid == 0) {
                unsigned cum = 0, bin = 0;
                for (; bin < 255u; ++bin) {
                    if (cum + hist[bin] > k) break;
                    cum += hist[bin];
                }
                sel[0] = (prefix << 8) | bin;
                sel[1] = k - cum;
            }
            __syncthreads();
            prefix = sel[0];
            k = sel[1];
        }
        if (tid == 0) {
            const float floor_db = vad_unkey(prefix), peak = vad_unkey(peak_key);
            const float lo = floor_db + margin_db, hi = peak - range_db, cap = peak - margin_db;
            const float m = lo > hi ? lo : hi;
            stats[3L * b] = floor_db;
            stats[3L * b + 1] = peak;
            stats[3L * b + 2] = m < cap ? m : cap;
        }
        __syncthreads();                                            // (peak_key and sel are the next row's too)
    }
}

// max over the threads before this one (-1 for thread 0) of one int per thread: Hillis-Steele over two LDS rows
static __device__ inline int vad_excl_scan_max(int v, int* buf) {
    const int tid = threadIdx.x;
    int *a = buf, *c = buf + VAD_ROW_THREADS;
    a[tid] = v;
    __syncthreads();
    for (int off = 1; off < VAD_ROW_THREADS; off <<= 1) {
        int x = a[tid];
        if (tid >= off) x = x > a[tid - off] ? x : a[tid - off];
        c[tid] = x;
        __syncthreads();
        int* s = a; a = c; c = s;
    }
    const int r = tid ? a[tid - 1] : -1;
    __syncthreads();
    return r;
}

// One pass over the frames [lo, hi) of a row in order, raw[t] = e[t] > thr && e[t] > min_db, the loads of VAD_UNROLL frames issued
// together.  st.pz follows the last frame with raw == 0; from STAGE 1 on st.last follows the last frame that is the mr-th or later
// of its run; STAGE 2 also stores st.last per frame.
struct VadWalk { int pz, last; };
template <int STAGE>
static __device__ __forceinline__ VadWalk vad_walk(const float* __restrict__ e, int lo, int hi, float thr, float min_db, int mr, VadWalk st,
                                                   int* out) {
    for (int t0 = lo; t0 < hi; t0 += VAD_UNROLL) {
        float v[VAD_UNROLL];
#pragma unroll
        for (int j = 0; j < VAD_UNROLL; ++j) v[j] = e[t0 + j < hi ? t0 + j : hi - 1];
#pragma unroll
        for (int j = 0; j < VAD_UNROLL; ++j) {
            const int t = t0 + j;
            if (t < hi) {
                if (!(v[j] > thr && v[j] > min_db)) st.pz = t;
                else if (STAGE >= 1 && t - st.pz >= mr) st.last = t;
                if (STAGE == 2) out[t] = st.last;
            }
        }
    }
    return st;
}

template <bool LEN_ARG>
__global__ __launch_bounds__(VAD_ROW_THREADS) void vad_flags_kernel(const float* __restrict__ energy, RowArgs len_arg,
                                                                    const int* __restrict__ len_dev, int B, int f_max, float min_db,
                                                                    int min_run, int hangover, const float* __restrict__ stats,
                                                                    unsigned char* __restrict__ speech, int* ws) {
    __shared__ int buf[2 * VAD_ROW_THREADS];
    const int tid = threadIdx.x;
    for (int b = blockIdx.x; b < B; b += gridDim.x) {
        int F = row_arg<LEN_ARG>(len_arg, len_dev, b);
        F = F < f_max ? F : f_max;
        F = F > 0 ? F : 0;
        const float* e = energy + (long)b * f_max;
        int* last_c = ws + (long)b * f_max;                         // [t]: the last frame <= t that is the min_run-th or later of its run
        const float thr = stats[3L * b + 2];
        const int mr = min_run > F ? F + 1 : min_run;               // (no run is longer than the row; keeps t + hangover + mr in an int)
        const int chunk = (F + VAD_ROW_THREADS - 1) / VAD_ROW_THREADS;
        const int lo = (long)tid * chunk < F ? tid * chunk : F, hi = lo + chunk < F ? lo + chunk : F;
        const int last0 = vad_walk<0>(e, lo, hi, thr, min_db, mr, VadWalk{-1, -1}, nullptr).pz;
        const int pz0 = vad_excl_scan_max(last0, buf);
        const int last1 = vad_walk<1>(e, lo, hi, thr, min_db, mr, VadWalk{pz0, -1}, nullptr).last;
        const int last_before = vad_excl_scan_max(last1, buf);
        vad_walk<2>(e, lo, hi, thr, min_db, mr, VadWalk{pz0, last_before}, last_c);
        __syncthreads();                                            // the workgroup's own global writes, read back below
        for (int t = tid; t < f_max; t += VAD_ROW_THREADS) {
            unsigned char s = 0;
            if (t < F) {
                long x = (long)t + hangover + mr - 1;
                x = x < F - 1 ? x : F - 1;
                const int p = last_c[x];
                s = p >= 0 && p >= t - hangover;
            }
            speech[(long)b * f_max + t] = s;
        }
        __syncthreads();
    }
}

// One span as the kernel reads it: its source row, its first sample and the words it really holds (already clipped on the host to
// the row's length and to w_out, never negative).
struct SpanArgs { int row[GS_ARGS_MAX], start[GS_ARGS_MAX], eff[GS_ARGS_MAX]; };

template <bool BY_ARG>
__global__ __launch_bounds__(GS_THREADS) void gather_spans_kernel(const float* __restrict__ pcm, SpanArgs args, const int* __restrict__ dev,
                                                                  int S, int n_max, int aligned, float* __restrict__ out, int w_out) {
    const long total = (long)S * w_out;
    const long e0 = 4 * ((long)blockIdx.x * GS_THREADS + threadIdx.x);
    if (e0 >= total) return;
    const int* d_row = dev, *d_start = dev + S, *d_eff = dev + 2L * S;
    float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    const int s0 = (int)(e0 / w_out), i0 = (int)(e0 - (long)s0 * w_out);
    bool done = false;
    if (i0 + 3 < w_out) {                                           // the four words lie in one span
        const int row = BY_ARG ? args.row[s0] : d_row[s0], start = BY_ARG ? args.start[s0] : d_start[s0];
        const int eff = BY_ARG ? args.eff[s0] : d_eff[s0];
        if (i0 >= eff) done = true;                                 // all padding
        else if (i0 + 3 < eff && ((start + i0) & 3) == 0 && (aligned == 2 || (aligned == 1 && row == 0))) {
            const f32x4 q = *reinterpret_cast<const f32x4*>(pcm + (long)row * n_max + start + i0);
            v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
            done = true;
        }
    }
    if (!done) {
        for (int j = 0; j < 4; ++j) {
            const long e = e0 + j;
            if (e >= total) break;
            const int s = (int)(e / w_out), i = (int)(e - (long)s * w_out);
            const int eff = BY_ARG ? args.eff[s] : d_eff[s];
            if (i < eff) {
                const int row = BY_ARG ? args.row[s] : d_row[s], start = BY_ARG ? args.start[s] : d_start[s];
                v[j] = pcm[(long)row * n_max + start + i];
            }
        }
    }
    if (e0 + 3 < total) {
        const f32x4 q = {v[0], v[1], v[2], v[3]};
        *reinterpret_cast<f32x4*>(out + e0) = q;
    } else {
        for (int j = 0; e0 + j < total; ++j) out[e0 + j] = v[j];   // the flat output's last one to three words
    }
}

// ---- the plan: the launch geometry as plain numbers (amdspeech.h: amdspeech_vad_plan_info).  The calls plan first and LAUNCH from
// the struct; amdspeech_vad_plan returns the same struct.  No device is needed.
static int plan_vad(int B, int n_max, int hop, VadPlan* p) {
    AS_CHECK_ARG(hop >= 1, "vad: hop %d must be at least 1", hop);
    AS_CHECK_ARG(B > 0 && n_max > 0, "vad: bad shape (B %d, n_max %d)", B, n_max);
    const int f_max = ceil_div(n_max, hop);
    AS_CHECK_ARG((long)B * f_max < (1L << 31), "vad: B %d x %d frames do not fit an int", B, f_max);
    p->f_max = f_max;
    // 16-byte loads need every block start 16-byte aligned: t * hop from a row base that is b * n_max words past an aligned pcm
    p->load_vec = (hop % 4 == 0 && (B == 1 || n_max % 4 == 0)) ? 4 : 1;
    p->frames_per_tile = VAD_TILE_FRAMES;
    p->tiles_per_row = ceil_div(f_max, VAD_TILE_FRAMES);
    p->workgroups = p->tiles_per_row * (B < VAD_GRID_ROWS ? B : VAD_GRID_ROWS);
    p->threads = VAD_THREADS;
    p->select_passes = VAD_SELECT_PASSES;
    p->row_workgroups = B < VAD_GRID_ROWS ? B : VAD_GRID_ROWS;
    p->row_threads = VAD_ROW_THREADS;
    p->meta_by_copy = B > ROW_ARGS_MAX ? 1 : 0;
    return AMDSPEECH_OK;
}

static int check_counts(const char* what, const int* v, int B, int top) {
    for (int b = 0; b < B; ++b)
        AS_CHECK_ARG(v[b] >= 0 && v[b] <= top, "%s[%d] = %d outside 0 .. %d", what, b, v[b], top);
    return AMDSPEECH_OK;
}

}  // namespace amdspeech

using namespace amdspeech;

extern "C" int amdspeech_vad_num_frames(int n_samples, int hop) {
    AS_CHECK_ARG(n_samples >= 0 && hop >= 1, "vad_num_frames: negative count or hop %d below 1", hop);
    return ceil_div(n_samples, hop);
}

extern "C" size_t amdspeech_vad_workspace_bytes(int B, int n_max, int hop) {
    if (B <= 0 || n_max <= 0 || hop < 1) return 0;
    return (size_t)B * (size_t)ceil_div(n_max, hop) * sizeof(int);
}

extern "C" int amdspeech_vad_plan(int B, int n_max, int hop, amdspeech_vad_plan_info* out) {
    AS_CHECK_ARG(out != nullptr, "vad_plan: null output");
    return plan_vad(B, n_max, hop, out);
}

extern "C" int amdspeech_vad_energy(void* stream, const float* pcm, const int* n_samples, int B, int n_max, int hop, float* energy_db,
                                    int f_max, void* /* ws: not read by this call */) {
    VadPlan pl;
    if (int rc = plan_vad(B, n_max, hop, &pl)) return rc;
    AS_CHECK_ARG(pcm && n_samples && energy_db, "vad_energy: null pointer");
    AS_CHECK_ARG(f_max >= pl.f_max, "vad_energy: f_max %d is below the %d frames of n_max %d at hop %d", f_max, pl.f_max, n_max, hop);
    AS_CHECK_ARG((long)B * f_max < (1L << 31), "vad_energy: B %d x f_max %d do not fit an int", B, f_max);
    AS_CHECK_ARG(pl.load_vec == 1 || (reinterpret_cast<uintptr_t>(pcm) & 15) == 0, "vad_energy: pcm must be 16-byte aligned when hop and the row pitch are multiples of 4");
    if (int rc = check_counts("vad_energy: n_samples", n_samples, B, n_max)) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const dim3 grid(ceil_div(f_max, VAD_TILE_FRAMES), B < VAD_GRID_ROWS ? B : VAD_GRID_ROWS), block(VAD_THREADS);
    return with_row_args(s, n_samples, B, [&](auto by_arg, const RowArgs& la, const int* d_len) {
        constexpr bool LEN_ARG = decltype(by_arg)::value;
        if (pl.load_vec == 4)
            hipLaunchKernelGGL((vad_energy_kernel<true, LEN_ARG>), grid, block, 0, s, pcm, la, d_len, B, n_max, hop, energy_db, f_max);
        else
            hipLaunchKernelGGL((vad_energy_kernel<false, LEN_ARG>), grid, block, 0, s, pcm, la, d_len, B, n_max, hop, energy_db, f_max);
        return hipGetLastError();
    });
}

extern "C" int amdspeech_vad_flags(void* stream, const float* energy_db, const int* n_frames, int B, int f_max, int percentile,
                                   float margin_db, float range_db, float min_db, int min_run, int hangover, unsigned char* speech,
                                   float* stats, void* ws) {
    AS_CHECK_ARG(B > 0 && f_max > 0 && (long)B * f_max < (1L << 31), "vad_flags: bad shape (B %d, f_max %d)", B, f_max);
    AS_CHECK_ARG(percentile >= 0 && percentile <= 100, "vad_flags: percentile %d outside 0 .. 100", percentile);
    AS_CHECK_ARG(min_run >= 1, "vad_flags: min_run %d must be at least 1", min_run);
    AS_CHECK_ARG(hangover >= 0 && hangover <= VAD_MAX_HANGOVER, "vad_flags: hangover %d outside 0 .. %d", hangover, VAD_MAX_HANGOVER);
    AS_CHECK_ARG(std::isfinite(margin_db) && std::isfinite(range_db) && std::isfinite(min_db),
                 "vad_flags: margin_db %g, range_db %g and min_db %g must be finite", margin_db, range_db, min_db);
    AS_CHECK_ARG(energy_db && n_frames && speech && stats && ws, "vad_flags: null pointer");
    AS_CHECK_ARG((reinterpret_cast<uintptr_t>(ws) & 3) == 0, "vad_flags: the workspace must be 4-byte aligned");
    if (int rc = check_counts("vad_flags: n_frames", n_frames, B, f_max)) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const dim3 grid(B < VAD_GRID_ROWS ? B : VAD_GRID_ROWS), block(VAD_ROW_THREADS);
    return with_row_args(s, n_frames, B, [&](auto by_arg, const RowArgs& la, const int* d_len) {
        constexpr bool LEN_ARG = decltype(by_arg)::value;
        hipLaunchKernelGGL((vad_select_kernel<LEN_ARG>), grid, block, 0, s, energy_db, la, d_len, B, f_max, percentile, margin_db, range_db,
                           stats);
        hipLaunchKernelGGL((vad_flags_kernel<LEN_ARG>), grid, block, 0, s, energy_db, la, d_len, B, f_max, min_db, min_run, hangover, stats,
                           speech, static_cast<int*>(ws));
        return hipGetLastError();
    });
}

extern "C" int amdspeech_gather_spans(void* stream, const float* pcm, const int* n_samples, int B, int n_max, const int* row,
                                      const int* start, const int* count, int S, float* out, int w_out) {
    AS_CHECK_ARG(B > 0 && n_max > 0, "gather_spans: bad shape (B %d, n_max %d)", B, n_max);
    AS_CHECK_ARG(S >= 0, "gather_spans: S = %d is negative", S);
    AS_CHECK_ARG(w_out >= 1, "gather_spans: w_out %d must be at least 1", w_out);
    AS_CHECK_ARG(pcm && n_samples, "gather_spans: null pointer");
    if (int rc = check_counts("gather_spans: n_samples", n_samples, B, n_max)) return rc;
    if (S == 0) return AMDSPEECH_OK;
    AS_CHECK_ARG(row && start && count && out, "gather_spans: null pointer");
    AS_CHECK_ARG((reinterpret_cast<uintptr_t>(out) & 15) == 0, "gather_spans: out must be 16-byte aligned");
    const long total = (long)S * w_out;
    AS_CHECK_ARG(total < (1L << 40), "gather_spans: %d spans of %d words are too many", S, w_out);
    for (int i = 0; i < S; ++i) {
        AS_CHECK_ARG(row[i] >= 0 && row[i] < B, "gather_spans: row[%d] = %d outside 0 .. %d", i, row[i], B - 1);
        AS_CHECK_ARG(start[i] >= 0 && count[i] >= 0, "gather_spans: span %d has a negative start %d or count %d", i, start[i], count[i]);
    }
    auto eff_of = [&](int i) {
        long e = (long)n_samples[row[i]] - start[i];
        e = e < count[i] ? e : count[i];
        e = e < w_out ? e : w_out;
        return (int)(e > 0 ? e : 0);
    };
    // 16-byte loads: 2 = every row base is 16-byte aligned, 1 = row 0 only (an odd row pitch), 0 = none (pcm itself is not)
    const int aligned = (reinterpret_cast<uintptr_t>(pcm) & 15) != 0 ? 0 : n_max % 4 == 0 ? 2 : 1;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)((total + 4L * GS_THREADS - 1) / (4L * GS_THREADS))), block(GS_THREADS);
    SpanArgs args;
    if (S <= GS_ARGS_MAX) {                                         // the spans travel as kernel arguments
        for (int i = 0; i < GS_ARGS_MAX; ++i) {
            args.row[i] = i < S ? row[i] : 0;
            args.start[i] = i < S ? start[i] : 0;
            args.eff[i] = i < S ? eff_of(i) : 0;
        }
        hipLaunchKernelGGL((gather_spans_kernel<true>), grid, block, 0, s, pcm, args, static_cast<const int*>(nullptr), S, n_max, aligned,
                           out, w_out);
        AS_CHECK_LAUNCH();
        return AMDSPEECH_OK;
    }
    // more spans than the argument block holds: through a device buffer of the call's own [3][S], and the call waits for the kernel
    // before it gives the buffer back (row_args.h: with_row_args does the same for rows)
    for (int i = 0; i < GS_ARGS_MAX; ++i) args.row[i] = args.start[i] = args.eff[i] = 0;
    int* host = static_cast<int*>(malloc(3 * (size_t)S * sizeof(int)));
    AS_CHECK_ARG(host != nullptr, "gather_spans: out of host memory for %d spans", S);
    for (int i = 0; i < S; ++i) {
        host[i] = row[i];
        host[S + i] = start[i];
        host[2L * S + i] = eff_of(i);
    }
    int* dev = nullptr;
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&dev), 3 * (size_t)S * sizeof(int));
    if (e == hipSuccess) e = hipMemcpyAsync(dev, host, 3 * (size_t)S * sizeof(int), hipMemcpyHostToDevice, s);
    if (e == hipSuccess) {
        hipLaunchKernelGGL((gather_spans_kernel<false>), grid, block, 0, s, pcm, args, static_cast<const int*>(dev), S, n_max, aligned, out,
                           w_out);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    const hipError_t ef = dev ? hipFree(dev) : hipSuccess;
    free(host);
    AS_CHECK_HIP(e);
    AS_CHECK_HIP(ef);
    return AMDSPEECH_OK;
}
