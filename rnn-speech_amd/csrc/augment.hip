// Noise and reverberation augmentation of training waveforms (amdspeech.h: amdspeech_reverb_rows, amdspeech_row_sumsq,
// amdspeech_noise_mix_rows, amdspeech_augment_draw), between the resampler and the front end.  No reference counterpart: an opt-in
// deviation, off unless a caller asks for it.  Host-side row values reach the kernels through row_args.h's write_ints.
#include "common.h"
#include "row_args.h"

#include <math.h>
#include <string.h>
#include <vector>

namespace amdspeech {

constexpr int AUG_MAX_ROWS = 65535;                  // grid y
constexpr int AUG_MAX_SAMPLES = 1 << 30;             // per row: tile starts and offset + t stay inside 32 bits
constexpr uint32_t AUG_DRAW_STREAM = 0x5C000000u;    // + 0 reverb apply, 1 RIR choice, 2 noise apply, 3 clip choice, 4 offset, 5 SNR

static bool ranges_overlap(const void* a, size_t a_bytes, const void* b, size_t b_bytes) {
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), a1 = a0 + a_bytes;
    const uintptr_t b0 = reinterpret_cast<uintptr_t>(b), b1 = b0 + b_bytes;
    return !(a1 <= b0 || b1 <= a0);
}

// ------------------------------------------------------------------------------------------------------------ reverberation
// out[b][t] = sum_k h[k] x[t + d - k] as a matrix product on the f32 matrix cores.  A workgroup owns RV_TILE = 1024 consecutive
// outputs of one row, t = t0 + 32 i + j:
//     Y[i][j] = sum_q X[i][q] G[q][j],   X[i][q] = xs[32 i + q],   G[q][j] = h[j + L - 1 - q]  (0 outside 0 .. L - 1),
// q = 0 .. L + 30, with xs the staged input span x[t0 + d - (L - 1) ..] (zeros outside 0 .. n - 1).  X is 32 overlapping windows of
// ONE staged span and G a Toeplitz band of ONE staged tap vector, so the operands of v_mfma_f32_32x32x2_f32 (lane l: row / column
// l & 31, k = l >> 5) are one ds_read_b32 each and nothing is materialised: 2 (L + 31) flops per output.
//   - xs is stored with one pad word per 32 (word p at p + p / 32): lanes i = 0 .. 31 read 33 words apart, no bank conflict;
//   - the taps are stored reversed and zero-framed, hr[w] = h[L + 30 - w] for w = 31 .. L + 30, so that G[q][j] = hr[q - j + 31]:
//     consecutive lanes read consecutive words;
//   - q runs in blocks of 32 (RV_KBLOCK); the workgroup's four waves take the blocks round-robin, each with its own accumulator, and
//     the four partial tiles are added through LDS (the span's words, once read) in wave order 0, 1, 2, 3: a fixed order, no
//     atomics, the same bits every call.
//     Every word either operand can reach is staged (zeros, never stale LDS): the zero frame multiplies finite numbers only;
//   - a row without an impulse response (index -1) is copied bit for bit, a tile at or past the row's length stores zeros: both
//     branches are uniform over the workgroup.  Every word of `out` is written, no input word at or past the row's length is read.
// The accumulation is an fmaf chain per accumulator (the f32 MFMA is exact f32), so every output is within (L + 2) 2^-24 sum |h x|.
// Measured (B 32 x 220,500 samples): 138 / 448 / 998 us per launch at 1024 / 4096 / 8192 taps against 547 / 1921 / 4171 us
// of the first correct version, a direct-form vector-ALU kernel (thread per 4 outputs, span and taps in LDS), on the same rows in the
// same profiler run; only this one is kept.
constexpr int RV_THREADS = 256, RV_TILE = 1024, RV_KBLOCK = 32, RV_TAPS_MAX = 8192;
constexpr int RV_RED_WORDS = 4 * 16 * 64;             // four partial tiles
constexpr int RV_LDS_MAX = 80 * 1024;                // (8192 taps need 70 KiB: two workgroups a CU)
constexpr int RV_META = 4;                          // ints per row: n, L (0: copy), delay, bank row
typedef amdspeech_reverb_rows_plan_info ReverbPlan;

static __host__ __device__ inline int rv_kblocks(int L) { return (L + 31 + RV_KBLOCK - 1) / RV_KBLOCK; }
static __host__ __device__ inline int rv_span(int L) { return RV_TILE - 32 + RV_KBLOCK * rv_kblocks(L); }      // staged input words
static __host__ __device__ inline int rv_pad(int p) { return p + (p >> 5); }
// words of the span's LDS region: the padded span rounded up to 4, at least the partial tiles that reuse it
static inline int rv_xs_words(int span) { const int w = (rv_pad(span) + 3) / 4 * 4; return w > RV_RED_WORDS ? w : RV_RED_WORDS; }

// meta: RV_META ints per row.  grid (tiles_per_row, B).  Dynamic LDS: xs_words = rv_xs_words(span_max) floats, then the taps.
__global__ __launch_bounds__(RV_THREADS) void reverb_rows_kernel(const float* __restrict__ x, const int* __restrict__ meta, int n_max,
                                                                 const float* __restrict__ bank, int taps_max, float* __restrict__ y,
                                                                 int xs_words) {
    extern __shared__ __attribute__((aligned(16))) float xs[];
    float (*red)[16][64] = reinterpret_cast<float (*)[16][64]>(xs);      // the partial tiles reuse the span's words
    float* hr = xs + xs_words;
    const int b = blockIdx.y, t0 = blockIdx.x * RV_TILE, tid = threadIdx.x;
    const int n = meta[RV_META * b], L = meta[RV_META * b + 1], d = meta[RV_META * b + 2], r = meta[RV_META * b + 3];
    const float* xb = x + (size_t)b * n_max;
    float* yb = y + (size_t)b * n_max;
    if (L == 0 || t0 >= n) {                             // copy row (bit patterns) or a tile of padding: zeros past the row
#pragma unroll
        for (int u = 0; u < RV_TILE / RV_THREADS; ++u) {
            const int t = t0 + u * RV_THREADS + tid;
            if (t < n_max) {
                unsigned v = 0u;
                if (L == 0 && t < n) v = reinterpret_cast<const unsigned*>(xb)[t];
                reinterpret_cast<unsigned*>(yb)[t] = v;
            }
        }
        return;
    }
    const int nblk = rv_kblocks(L), span = rv_span(L);
    const long s0 = (long)t0 + d - (L - 1);               // row position of xs word 0
    for (int u = tid; u < span; u += RV_THREADS) {
        const long p = s0 + u;
        xs[rv_pad(u)] = (p >= 0 && p < n) ? xb[p] : 0.0f;
    }
    const float* h = bank + (size_t)r * taps_max;
    for (int w = tid; w < RV_KBLOCK * nblk + 32; w += RV_THREADS) {
        const int k = L + 30 - w;
        hr[w] = (k >= 0 && k < L) ? h[k] : 0.0f;
    }
    __syncthreads();
    const int wave = tid >> 6, lane = tid & 63, half = lane >> 5, col = lane & 31;
    f32x16 acc;
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] = 0.0f;
    const float* xa = xs + 33 * col + half;               // X[i = col][q]: word 32 i + q at 33 i + q + q / 32
    const float* hb = hr + 31 - col + half;               // G[q][j = col]: hr[q - j + 31]
    for (int blk = wave; blk < nblk; blk += 4) {
        const float* xq = xa + 33 * blk;                  // q = 32 blk + 2 s + half: q / 32 == blk for every s
        const float* hq = hb + 32 * blk;
#pragma unroll
        for (int s = 0; s < RV_KBLOCK / 2; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(xq[2 * s], hq[2 * s], acc, 0, 0, 0);
    }
    __syncthreads();                                      // (every wave has read its last span word)
#pragma unroll
    for (int e = 0; e < 16; ++e) red[wave][e][lane] = acc[e];
    __syncthreads();
    // wave w finishes accumulator words 4 w .. 4 w + 3: tile row i = (e & 3) + 8 (e >> 2) + 4 half, column j = col
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int e = 4 * wave + u;
        const float v = ((red[0][e][lane] + red[1][e][lane]) + red[2][e][lane]) + red[3][e][lane];
        const int t = t0 + 32 * ((e & 3) + 8 * (e >> 2) + 4 * half) + col;
        if (t < n_max) yb[t] = t < n ? v : 0.0f;
    }
}

// ---- the plan: checks and launch geometry (amdspeech.h: amdspeech_reverb_rows_plan_info).  amdspeech_reverb_rows plans first and
// LAUNCHES from the struct; amdspeech_reverb_rows_plan returns the same struct.  No device.
static int plan_reverb_rows(const int* n_samples, int B, int n_max, const int* rir_taps, const int* rir_delay, int R, int taps_max,
                            const int* rir_index, ReverbPlan* p) {
    AS_CHECK_ARG(n_samples && rir_taps && rir_delay && rir_index && p, "reverb_rows: null pointer");
    AS_CHECK_ARG(B > 0 && n_max > 0 && R > 0 && taps_max > 0, "reverb_rows: bad shape (B %d, n_max %d, R %d, taps_max %d)", B, n_max, R,
                 taps_max);
    AS_CHECK_ARG(B <= AUG_MAX_ROWS, "reverb_rows: B %d above %d rows", B, AUG_MAX_ROWS);
    AS_CHECK_ARG(n_max <= AUG_MAX_SAMPLES, "reverb_rows: n_max %d above 2^30", n_max);
    AS_CHECK_ARG(taps_max <= RV_TAPS_MAX, "reverb_rows: taps_max %d above %d", taps_max, RV_TAPS_MAX);
    for (int r = 0; r < R; ++r) {
        AS_CHECK_ARG(rir_taps[r] >= 1 && rir_taps[r] <= taps_max, "reverb_rows: rir_taps[%d] = %d outside 1 .. taps_max %d", r, rir_taps[r],
                     taps_max);
        AS_CHECK_ARG(rir_delay[r] >= 0 && rir_delay[r] < rir_taps[r], "reverb_rows: rir_delay[%d] = %d outside 0 .. taps - 1 = %d", r,
                     rir_delay[r], rir_taps[r] - 1);
    }
    int taps = 0, copies = 0;
    for (int b = 0; b < B; ++b) {
        AS_CHECK_ARG(n_samples[b] >= 0 && n_samples[b] <= n_max, "reverb_rows: n_samples[%d] = %d outside 0 .. n_max %d", b, n_samples[b],
                     n_max);
        AS_CHECK_ARG(rir_index[b] >= -1 && rir_index[b] < R, "reverb_rows: rir_index[%d] = %d outside -1 .. R - 1 = %d", b, rir_index[b],
                     R - 1);
        if (rir_index[b] < 0) ++copies;
        else if (n_samples[b] > 0 && rir_taps[rir_index[b]] > taps) taps = rir_taps[rir_index[b]];
    }
    p->tile = RV_TILE;
    p->tiles_per_row = ceil_div(n_max, RV_TILE);
    p->workgroups = p->tiles_per_row * B;
    p->taps = taps;
    p->span_max = taps > 0 ? rv_span(taps) : 0;
    p->k_chunk = RV_KBLOCK;
    p->k_chunks = taps > 0 ? rv_kblocks(taps) : 0;
    p->lds_bytes = taps > 0 ? (rv_xs_words(p->span_max) + RV_KBLOCK * p->k_chunks + 32) * 4 : 0;
    p->copy_rows = copies;
    p->meta_launches = ceil_div((long)RV_META * B, 2 * ROW_ARGS_MAX);
    return AMDSPEECH_OK;
}

// --------------------------------------------------------------------------------------------------------- sum of squares
// sumsq[b] = sum_{t < n} x[b][t]^2 in float64, the same bits every call and whatever the batch around the row: the row is cut into
// tiles of SS_TILE samples; workgroup (s, b) takes tiles s, s + SS_SPLIT, .. in that order, thread i adding the squares of words
// i, i + 256, .. of each tile to ITS double; the 256 doubles are added in a fixed tree, and a second one-block-per-row launch adds
// the SS_SPLIT partial sums in a fixed tree.  Nothing depends on n_max, B or the launch order; no word at or past n is read.
constexpr int SS_THREADS = 256, SS_TILE = 4096, SS_SPLIT = 64;

template <int N>
static __device__ __forceinline__ double tree_sum(double* s, double v, int tid) {      // N a power of two <= blockDim.x; all threads call
    s[tid] = v;
    __syncthreads();
#pragma unroll
    for (int w = N / 2; w > 0; w >>= 1) {
        if (tid < w) s[tid] += s[tid + w];
        __syncthreads();
    }
    return s[0];
}

__global__ __launch_bounds__(SS_THREADS) void row_sumsq_partial_kernel(const float* __restrict__ x, const int* __restrict__ meta,
                                                                       int n_max, double* __restrict__ partial) {
    __shared__ double s[SS_THREADS];
    const int b = blockIdx.y, tid = threadIdx.x, n = meta[b];
    const float* xb = x + (size_t)b * n_max;
    double acc = 0.0;
    for (long base = (long)blockIdx.x * SS_TILE; base < n; base += (long)SS_SPLIT * SS_TILE) {
#pragma unroll 4
        for (int u = 0; u < SS_TILE / SS_THREADS; ++u) {
            const long t = base + u * SS_THREADS + tid;
            if (t < n) { const double v = (double)xb[t]; acc = fma(v, v, acc); }
        }
    }
    const double total = tree_sum<SS_THREADS>(s, acc, tid);
    if (tid == 0) partial[(size_t)b * SS_SPLIT + blockIdx.x] = total;
}

__global__ __launch_bounds__(SS_SPLIT) void row_sumsq_final_kernel(const double* __restrict__ partial, double* __restrict__ out) {
    __shared__ double s[SS_SPLIT];
    const double total = tree_sum<SS_SPLIT>(s, partial[(size_t)blockIdx.x * SS_SPLIT + threadIdx.x], threadIdx.x);
    if (threadIdx.x == 0) out[blockIdx.x] = total;
}

// ------------------------------------------------------------------------------------------------------------- noise mix
// out[b][t] = fmaf(g, noise_m[(offset + t) mod len_m], x[b][t]), t < n; g in double from the two sums of squares and the host's
// 10^(-snr / 100), rounded once.  One word in, one word out at the same index: in place is safe.  Out of place the words past n are
// written +0.0f; in place they are left alone.
constexpr int NM_THREADS = 256, NM_TILE = 1024;
constexpr int NM_META = 6;                           // ints per row: n, clip (-1: none), offset, len, lo / hi word of 10^(-snr/100)
typedef amdspeech_noise_mix_rows_plan_info NoisePlan;

__global__ __launch_bounds__(NM_THREADS) void noise_mix_rows_kernel(const float* __restrict__ x, const int* __restrict__ meta, int n_max,
                                                                    const float* __restrict__ bank, int m_max,
                                                                    const double* __restrict__ noise_sumsq,
                                                                    const double* __restrict__ row_sumsq, float* __restrict__ y,
                                                                    int in_place) {
    const int b = blockIdx.y, t0 = blockIdx.x * NM_TILE, tid = threadIdx.x;
    const int* mb = meta + NM_META * b;
    const int n = mb[0], m = mb[1];
    const unsigned offset = (unsigned)mb[2], len = (unsigned)mb[3];
    const unsigned* xb = reinterpret_cast<const unsigned*>(x) + (size_t)b * n_max;
    unsigned* yb = reinterpret_cast<unsigned*>(y) + (size_t)b * n_max;
    bool mix = false;
    float g = 0.0f;
    if (m >= 0 && n > 0 && t0 < n) {
        const double rs = row_sumsq[b], ns = noise_sumsq[m];
        if (rs > 0.0 && ns > 0.0) {
            const double scale = __hiloint2double(mb[5], mb[4]);
            g = (float)sqrt((rs / (double)n) / (ns / (double)len) * scale);
            mix = true;
        }
    }
    if (!mix && in_place) return;
    const float* nz = bank + (size_t)(m < 0 ? 0 : m) * m_max;
#pragma unroll
    for (int u = 0; u < NM_TILE / NM_THREADS; ++u) {
        const int t = t0 + u * NM_THREADS + tid;
        if (t >= n_max) continue;
        if (t >= n) {
            if (!in_place) yb[t] = 0u;
            continue;
        }
        unsigned v = xb[t];
        if (mix) v = __float_as_uint(fmaf(g, nz[(offset + (unsigned)t) % len], __uint_as_float(v)));
        yb[t] = v;
    }
}

static int plan_noise_mix_rows(const int* n_samples, int B, int n_max, const int* noise_len, int M, int m_max, const int* noise_index,
                               const int* noise_offset, const int* snr_decidb, NoisePlan* p) {
    AS_CHECK_ARG(n_samples && noise_len && noise_index && noise_offset && snr_decidb && p, "noise_mix_rows: null pointer");
    AS_CHECK_ARG(B > 0 && n_max > 0 && M > 0 && m_max > 0, "noise_mix_rows: bad shape (B %d, n_max %d, M %d, m_max %d)", B, n_max, M, m_max);
    AS_CHECK_ARG(B <= AUG_MAX_ROWS, "noise_mix_rows: B %d above %d rows", B, AUG_MAX_ROWS);
    AS_CHECK_ARG(n_max <= AUG_MAX_SAMPLES && m_max <= AUG_MAX_SAMPLES, "noise_mix_rows: n_max %d or m_max %d above 2^30", n_max, m_max);
    for (int m = 0; m < M; ++m)
        AS_CHECK_ARG(noise_len[m] >= 1 && noise_len[m] <= m_max, "noise_mix_rows: noise_len[%d] = %d outside 1 .. m_max %d", m, noise_len[m],
                     m_max);
    int copies = 0;
    for (int b = 0; b < B; ++b) {
        AS_CHECK_ARG(n_samples[b] >= 0 && n_samples[b] <= n_max, "noise_mix_rows: n_samples[%d] = %d outside 0 .. n_max %d", b,
                     n_samples[b], n_max);
        const int m = noise_index[b];
        AS_CHECK_ARG(m >= -1 && m < M, "noise_mix_rows: noise_index[%d] = %d outside -1 .. M - 1 = %d", b, m, M - 1);
        if (m < 0) { ++copies; continue; }
        AS_CHECK_ARG(noise_offset[b] >= 0 && noise_offset[b] < noise_len[m], "noise_mix_rows: noise_offset[%d] = %d outside 0 .. len - 1 = %d",
                     b, noise_offset[b], noise_len[m] - 1);
        AS_CHECK_ARG(snr_decidb[b] >= -200 && snr_decidb[b] <= 600, "noise_mix_rows: snr_decidb[%d] = %d outside -200 .. 600", b,
                     snr_decidb[b]);
    }
    p->tile = NM_TILE;
    p->tiles_per_row = ceil_div(n_max, NM_TILE);
    p->workgroups = p->tiles_per_row * B;
    p->lds_bytes = 0;
    p->copy_rows = copies;
    p->meta_launches = ceil_div((long)NM_META * B, 2 * ROW_ARGS_MAX);
    return AMDSPEECH_OK;
}

}  // namespace amdspeech

using namespace amdspeech;

extern "C" size_t amdspeech_reverb_rows_workspace_bytes(int B) { return B > 0 ? align_up((size_t)RV_META * B * 4, 256) : 0; }

extern "C" int amdspeech_reverb_rows_plan(const int* n_samples, int B, int n_max, const int* rir_taps, const int* rir_delay, int R,
                                          int taps_max, const int* rir_index, amdspeech_reverb_rows_plan_info* out) {
    AS_CHECK_ARG(out != nullptr, "reverb_rows_plan: null output");
    return plan_reverb_rows(n_samples, B, n_max, rir_taps, rir_delay, R, taps_max, rir_index, out);
}

extern "C" int amdspeech_reverb_rows(void* stream, const float* pcm, const int* n_samples, int B, int n_max, const float* rir_bank,
                                     const int* rir_taps, const int* rir_delay, int R, int taps_max, const int* rir_index, float* out,
                                     void* ws) {
    hipStream_t s = static_cast<hipStream_t>(stream);
    AS_CHECK_ARG(pcm && rir_bank && out && ws, "reverb_rows: null pointer");
    ReverbPlan pl;
    if (int rc = plan_reverb_rows(n_samples, B, n_max, rir_taps, rir_delay, R, taps_max, rir_index, &pl)) return rc;
    AS_CHECK_ARG(!ranges_overlap(pcm, (size_t)B * n_max * 4, out, (size_t)B * n_max * 4), "reverb_rows: pcm and out overlap");
    AS_CHECK_ARG(!ranges_overlap(rir_bank, (size_t)R * taps_max * 4, out, (size_t)B * n_max * 4), "reverb_rows: rir_bank and out overlap");
    std::vector<int> host((size_t)RV_META * B);
    for (int b = 0; b < B; ++b) {
        const int r = rir_index[b];
        host[RV_META * b] = n_samples[b];
        host[RV_META * b + 1] = r < 0 ? 0 : rir_taps[r];
        host[RV_META * b + 2] = r < 0 ? 0 : rir_delay[r];
        host[RV_META * b + 3] = r < 0 ? 0 : r;
    }
    int* meta = static_cast<int*>(ws);
    write_ints(s, meta, host.data(), RV_META * B);
    static unsigned long long lds_seen = 0;
    if (DeviceOnce once{&lds_seen}) {
        AS_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(reverb_rows_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                         RV_LDS_MAX));
        once.done();
    }
    const int xs_words = rv_xs_words(pl.span_max);
    hipLaunchKernelGGL(reverb_rows_kernel, dim3(pl.tiles_per_row, B), dim3(RV_THREADS), (size_t)pl.lds_bytes, s, pcm, meta, n_max, rir_bank,
                       taps_max, out, xs_words);
    AS_CHECK_LAUNCH();
    return AMDSPEECH_OK;
}

extern "C" size_t amdspeech_row_sumsq_workspace_bytes(int B) {
    return B > 0 ? align_up((size_t)B * SS_SPLIT * sizeof(double), 256) + align_up((size_t)B * 4, 256) : 0;
}

extern "C" int amdspeech_row_sumsq(void* stream, const float* pcm, const int* n_samples, int B, int n_max, double* sumsq, void* ws) {
    hipStream_t s = static_cast<hipStream_t>(stream);
    AS_CHECK_ARG(pcm && n_samples && sumsq && ws, "row_sumsq: null pointer");
    AS_CHECK_ARG(B > 0 && n_max > 0, "row_sumsq: bad shape (B %d, n_max %d)", B, n_max);
    AS_CHECK_ARG(B <= AUG_MAX_ROWS, "row_sumsq: B %d above %d rows", B, AUG_MAX_ROWS);
    AS_CHECK_ARG(n_max <= AUG_MAX_SAMPLES, "row_sumsq: n_max %d above 2^30", n_max);
    for (int b = 0; b < B; ++b)
        AS_CHECK_ARG(n_samples[b] >= 0 && n_samples[b] <= n_max, "row_sumsq: n_samples[%d] = %d outside 0 .. n_max %d", b, n_samples[b], n_max);
    double* partial = static_cast<double*>(ws);
    int* meta = reinterpret_cast<int*>(static_cast<char*>(ws) + align_up((size_t)B * SS_SPLIT * sizeof(double), 256));
    write_ints(s, meta, n_samples, B);
    hipLaunchKernelGGL(row_sumsq_partial_kernel, dim3(SS_SPLIT, B), dim3(SS_THREADS), 0, s, pcm, meta, n_max, partial);
    hipLaunchKernelGGL(row_sumsq_final_kernel, dim3(B), dim3(SS_SPLIT), 0, s, partial, sumsq);
    AS_CHECK_LAUNCH();
    return AMDSPEECH_OK;
}

extern "C" size_t amdspeech_noise_mix_rows_workspace_bytes(int B) { return B > 0 ? align_up((size_t)NM_META * B * 4, 256) : 0; }

extern "C" int amdspeech_noise_mix_rows_plan(const int* n_samples, int B, int n_max, const int* noise_len, int M, int m_max,
                                             const int* noise_index, const int* noise_offset, const int* snr_decidb,
                                             amdspeech_noise_mix_rows_plan_info* out) {
    AS_CHECK_ARG(out != nullptr, "noise_mix_rows_plan: null output");
    return plan_noise_mix_rows(n_samples, B, n_max, noise_len, M, m_max, noise_index, noise_offset, snr_decidb, out);
}

extern "C" int amdspeech_noise_mix_rows(void* stream, const float* pcm, const int* n_samples, int B, int n_max, const float* noise_bank,
                                        const int* noise_len, const double* noise_sumsq, int M, int m_max, const double* row_sumsq,
                                        const int* noise_index, const int* noise_offset, const int* snr_decidb, float* out, void* ws) {
    hipStream_t s = static_cast<hipStream_t>(stream);
    AS_CHECK_ARG(pcm && noise_bank && noise_sumsq && row_sumsq && out && ws, "noise_mix_rows: null pointer");
    NoisePlan pl;
    if (int rc = plan_noise_mix_rows(n_samples, B, n_max, noise_len, M, m_max, noise_index, noise_offset, snr_decidb, &pl)) return rc;
    const size_t bytes = (size_t)B * n_max * 4;
    AS_CHECK_ARG(out == pcm || !ranges_overlap(pcm, bytes, out, bytes), "noise_mix_rows: pcm and out overlap in part");
    AS_CHECK_ARG(!ranges_overlap(noise_bank, (size_t)M * m_max * 4, out, bytes), "noise_mix_rows: noise_bank and out overlap");
    std::vector<int> host((size_t)NM_META * B);
    for (int b = 0; b < B; ++b) {
        const int m = noise_index[b];
        const double scale = m < 0 ? 0.0 : pow(10.0, -(double)snr_decidb[b] / 100.0);
        int words[2];
        memcpy(words, &scale, sizeof scale);
        int* hb = &host[(size_t)NM_META * b];
        hb[0] = n_samples[b];
        hb[1] = m;
        hb[2] = m < 0 ? 0 : noise_offset[b];
        hb[3] = m < 0 ? 1 : noise_len[m];
        hb[4] = words[0];
        hb[5] = words[1];
    }
    int* meta = static_cast<int*>(ws);
    write_ints(s, meta, host.data(), NM_META * B);
    hipLaunchKernelGGL(noise_mix_rows_kernel, dim3(pl.tiles_per_row, B), dim3(NM_THREADS), 0, s, pcm, meta, n_max, noise_bank, m_max,
                       noise_sumsq, row_sumsq, out, out == pcm ? 1 : 0);
    AS_CHECK_LAUNCH();
    return AMDSPEECH_OK;
}

extern "C" int amdspeech_augment_draw(unsigned long long seed, unsigned long long index, int reverb_permille, int R, int noise_permille,
                                      int M, const int* noise_len, int snr_lo_decidb, int snr_hi_decidb, int* out) {
    AS_CHECK_ARG(out != nullptr, "augment_draw: null output");
    AS_CHECK_ARG(reverb_permille >= 0 && reverb_permille <= 1000 && noise_permille >= 0 && noise_permille <= 1000,
                 "augment_draw: probabilities %d, %d permille outside 0 .. 1000", reverb_permille, noise_permille);
    AS_CHECK_ARG(R >= 0 && M >= 0, "augment_draw: negative bank size (R %d, M %d)", R, M);
    AS_CHECK_ARG(M == 0 || noise_len != nullptr, "augment_draw: null noise_len");
    AS_CHECK_ARG(snr_lo_decidb >= -200 && snr_lo_decidb <= snr_hi_decidb && snr_hi_decidb <= 600,
                 "augment_draw: snr range %d .. %d decidb outside -200 .. 600 or empty", snr_lo_decidb, snr_hi_decidb);
    for (int m = 0; m < M; ++m) AS_CHECK_ARG(noise_len[m] >= 1, "augment_draw: noise_len[%d] = %d below 1", m, noise_len[m]);
    const uint32_t idx = (uint32_t)index + (uint32_t)(index >> 32) * 0x9E3779B1u;
    auto draw = [&](uint32_t which, uint64_t count) { return (int)(((uint64_t)random24(seed, AUG_DRAW_STREAM + which, idx) * count) >> 24); };
    out[0] = out[1] = -1;
    out[2] = out[3] = 0;
    if (R > 0 && draw(0, 1000) < reverb_permille) out[0] = draw(1, (uint64_t)R);
    if (M > 0 && draw(2, 1000) < noise_permille) {
        out[1] = draw(3, (uint64_t)M);
        out[2] = draw(4, (uint64_t)noise_len[out[1]]);
        out[3] = snr_lo_decidb + draw(5, (uint64_t)(snr_hi_decidb - snr_lo_decidb + 1));
    }
    return AMDSPEECH_OK;
}
