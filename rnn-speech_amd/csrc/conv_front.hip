// Strided time-frequency convolution between the features and the input Linear (amdspeech.h: amdspeech_conv2d_fwd / _bwd): one
// learned filter bank of C channels over (time, frequency) with "same" padding, strides st x sf and Deep Speech 2's clipped ReLU.
// No reference counterpart (an opt-in deviation); off at conv_channels 0, where no caller makes these calls.
//
//   x [T][B][G][F],  w [K = G kt kf][C] (row k = (g kt + i) kf + j),  bias [C],  y [T'][B][F'][C],  T' = ceil(T / st), F' = ceil(F / sf)
//   Lb = min(max(lengths[b], 0), T),  L'b = ceil(Lb / st)
//   pre[t'][b][f'][c] = bias[c] + sum_{g,i,j} w[k][c] x[t' st + i - pt][b][g][f' sf + j - pf]     (source frame in 0 .. Lb-1, bin in 0 .. F-1)
//   y = min(max(pre, 0), 20) for t' < L'b, 0 past it;   dw[k][c] += sum patch_k dy mask,  db[c] += sum dy mask,  mask = 0 < y < 20
//
// Both passes are matrix products on v_mfma_f32_16x16x4_f32 (exact f32) over ONE tile geometry: a workgroup (4 waves) takes `tile_t`
// output frames x all F' output bins of one row b, at most CF_TILE_M = 128 output positions, flattened m = t'_local F' + f'.  It
// stages the source span of the tile once in LDS -- (tile_t - 1) st + kt frames of G (F + 2 pf) words, zeros for the frequency border
// and for frames outside 0 .. Lb-1 (those are never loaded) -- so that the operand gather is patch[base(m) + off(k)] with no branch:
// base(m) = t'_local st rowW + f' sf, off(k) = i rowW + g (F + 2 pf) + j.
//   conv2d_fwd_kernel<NB>    M = positions (32 per wave: two 16-row blocks), N = C = 16 NB, K = (g, i, j) padded to 4 with zero weights.
//                            The weights pass through LDS in chunks of `k_chunk` rows ([k][C] with the row stride padded against
//                            bank conflicts): ONE chunk when the whole [k_pad][C] fits beside the patch ("resident"), else 64 rows
//                            at a time, re-read per workgroup from L2 ("streamed").  Epilogue: + bias, clip, zeros at t' >= L'b.
//   conv2d_dw_kernel<NB>     M = k rows (a wave holds 4 blocks of 16, a workgroup 256 rows: grid.y covers K + 1), N = C, the
//                            reduction runs over the positions.  Row K is the constant 1: the bias gradient is that row of the same
//                            product.  Workgroup p of `dw_partials` walks the tiles p, p + dw_partials, ... (index t'-tile * B + b),
//                            staging the patch and dy * mask of each, and writes ONE partial [K + 1][C] tile -- every word the
//                            second stage reads, so the workspace needs no fill.
//   conv2d_reduce_kernel     dw / db += the partials: CF_SLICES threads per element each sum a contiguous run in index order, the
//                            slices are added in slice order, one add into the output.
// No atomics: y, dw and db are bit-identical from run to run.
#include "common.h"

namespace amdspeech {

constexpr int CF_THREADS = 256;           // 4 waves
constexpr int CF_TILE_M = 128;            // output positions per tile: 4 waves x 2 blocks of 16 (fwd) = 32 reduction steps of 4 (bwd)
constexpr int CF_K_STREAM = 64;           // weight rows per LDS chunk when they are streamed
constexpr int CF_LDS_BUDGET = 64 * 1024;  // what a kernel gets unasked; two workgroups per CU
constexpr int CF_KROWS_WG = 256;          // k rows of one dw workgroup: 4 waves x 4 blocks x 16
constexpr int CF_DW_TARGET_WGS = 512;
constexpr int CF_SLICES = 8;
constexpr int CF_RED_COLS = 32;
constexpr int CF_MAX_F = 128, CF_MAX_G = 3, CF_MAX_KT = 11, CF_MAX_KF = 41, CF_MAX_STRIDE = 4;

typedef amdspeech_conv2d_plan_info CfPlan;

struct CfDims {
    int T, B, G, F, C, kt, kf, st, sf;
    int T_out, F_out, K, k_pad, pt, pf, Fp, rowW, span, tile_t, w_stride, k_chunk;
};

static __host__ __device__ inline int cf_w_stride(int C) { return C == 16 ? 16 : C <= 48 ? 48 : 80; }   // stride mod 64 in {16, 48}: 4 k rows x 16 channels hit 64 banks

// The source span of tile (t0 .. t0 + tile_t - 1, row b) into LDS: patch[p][g][F + 2 pf], frame p = source frame t0 st - pt + p.
static __device__ inline void cf_stage_patch(const CfDims& d, const float* __restrict__ x, int b, int t0, int Lb, float* patch) {
    const int n = d.span * d.rowW;
    const int src0 = t0 * d.st - d.pt;
    const long D = (long)d.G * d.F;
    for (int idx = threadIdx.x; idx < n; idx += CF_THREADS) {
        const int p = idx / d.rowW, r = idx - p * d.rowW;
        const int g = r / d.Fp, bin = r - g * d.Fp - d.pf;
        const int ts = src0 + p;
        float v = 0.f;
        if (ts >= 0 && ts < Lb && bin >= 0 && bin < d.F) v = x[((long)ts * d.B + b) * D + (long)g * d.F + bin];
        patch[idx] = v;
    }
}

static __device__ inline int cf_row_len(const int* __restrict__ lengths, int b, int T) {
    int n = lengths[b];
    n = n < T ? n : T;
    return n > 0 ? n : 0;
}

template <int NB>
__global__ __launch_bounds__(CF_THREADS) void conv2d_fwd_kernel(CfDims d, const float* __restrict__ x, const float* __restrict__ w,
                                                                const float* __restrict__ bias, const int* __restrict__ lengths,
                                                                float* __restrict__ y, int* __restrict__ lengths_out) {
    extern __shared__ __attribute__((aligned(16))) float cf_lds[];
    float* patch = cf_lds;                                           // [span][rowW]
    int* koff = reinterpret_cast<int*>(cf_lds + d.span * d.rowW);    // [k_pad]
    float* wl = cf_lds + d.span * d.rowW + d.k_pad;                  // [k_chunk][w_stride]
    const int b = blockIdx.y, t0 = blockIdx.x * d.tile_t;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int Lb = cf_row_len(lengths, b, d.T);
    const int Lo = (Lb + d.st - 1) / d.st;
    if (blockIdx.x == 0 && threadIdx.x == 0) lengths_out[b] = Lo;
    const int t1 = t0 + d.tile_t < d.T_out ? t0 + d.tile_t : d.T_out;
    const long ystride = (long)d.F_out * d.C;
    if (t0 >= Lo) {                                                  // (uniform) the whole tile lies past the row: zeros, nothing is read
        const long n = (long)(t1 - t0) * ystride;
        for (long e = threadIdx.x; e < n; e += CF_THREADS) {
            const long tl = e / ystride;
            y[((long)(t0 + tl) * d.B + b) * ystride + (e - tl * ystride)] = 0.f;
        }
        return;
    }
    cf_stage_patch(d, x, b, t0, Lb, patch);
    for (int k = threadIdx.x; k < d.k_pad; k += CF_THREADS) {
        int o = 0;
        if (k < d.K) {
            const int j = k % d.kf, gi = k / d.kf, i = gi % d.kt, g = gi / d.kt;
            o = i * d.rowW + g * d.Fp + j;
        }
        koff[k] = o;
    }
    // this wave's two blocks of 16 positions; lane's A rows are m = block * 16 + (lane & 15)
    const int n_pos = d.tile_t * d.F_out;
    int base[2];
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        const int m = (wave * 2 + q) * 16 + (lane & 15);
        base[q] = 0;
        if (m < n_pos) {
            const int tl = m / d.F_out, f = m - tl * d.F_out;
            base[q] = tl * d.st * d.rowW + f * d.sf;
        }
    }
    f32x4 acc[2][NB];
#pragma unroll
    for (int q = 0; q < 2; ++q)
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) acc[q][nb] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int kq = lane >> 4, col = lane & 15;
    for (int c0 = 0; c0 < d.k_pad; c0 += d.k_chunk) {
        const int rows = d.k_pad - c0 < d.k_chunk ? d.k_pad - c0 : d.k_chunk;     // (a multiple of 4)
        __syncthreads();                                             // the previous chunk has been read (first pass: nothing)
        for (int e = threadIdx.x; e < rows * d.C; e += CF_THREADS) {
            const int kk = e / d.C, c = e - kk * d.C;
            wl[kk * d.w_stride + c] = c0 + kk < d.K ? w[(long)(c0 + kk) * d.C + c] : 0.f;
        }
        __syncthreads();                                             // (first pass: the patch and the offsets too)
        if (wave * 32 < n_pos) {                                     // (uniform per wave; no barrier inside)
            for (int s = 0; s < rows; s += 4) {
                const int ko = koff[c0 + s + kq];
                const float a0 = patch[base[0] + ko], a1 = patch[base[1] + ko];
                const float* wr = wl + (s + kq) * d.w_stride + col;
#pragma unroll
                for (int nb = 0; nb < NB; ++nb) {
                    const float bv = wr[nb * 16];
                    acc[0][nb] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, bv, acc[0][nb], 0, 0, 0);
                    acc[1][nb] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, bv, acc[1][nb], 0, 0, 0);
                }
            }
        }
    }
    // epilogue: register r of lane l is position block * 16 + (l >> 4) * 4 + r, channel nb * 16 + (l & 15)
#pragma unroll
    for (int q = 0; q < 2; ++q) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int m = (wave * 2 + q) * 16 + kq * 4 + r;
            if (m >= n_pos) continue;
            const int tl = m / d.F_out, f = m - tl * d.F_out;
            const int t = t0 + tl;
            if (t >= d.T_out) continue;
            float* out = y + ((long)t * d.B + b) * ystride + (long)f * d.C + col;
#pragma unroll
            for (int nb = 0; nb < NB; ++nb) {
                const float pre = acc[q][nb][r] + bias[nb * 16 + col];
                out[nb * 16] = t < Lo ? fminf(fmaxf(pre, 0.f), 20.f) : 0.f;
            }
        }
    }
}

template <int NB>
__global__ __launch_bounds__(CF_THREADS) void conv2d_dw_kernel(CfDims d, const float* __restrict__ x, const float* __restrict__ y,
                                                               const float* __restrict__ dy, const int* __restrict__ lengths,
                                                               int n_tiles, int n_part, int k_rows, float* __restrict__ part) {
    extern __shared__ __attribute__((aligned(16))) float cf_lds[];
    float* patch = cf_lds;                                           // [span][rowW]
    int* posbase = reinterpret_cast<int*>(cf_lds + d.span * d.rowW); // [CF_TILE_M]
    float* gl = cf_lds + d.span * d.rowW + CF_TILE_M;                // [CF_TILE_M][w_stride]   dy * mask
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int kq = lane >> 4, col = lane & 15;
    const int n_pos = d.tile_t * d.F_out;
    const int steps = (n_pos + 3) / 4;
    const long ystride = (long)d.F_out * d.C;
    // this wave's 4 blocks of 16 k rows; lane's A rows are k = block * 16 + (lane & 15)
    const int kb0 = (blockIdx.y * CF_KROWS_WG) / 16 + wave * 4;
    int koff[4];
    bool one[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int k = (kb0 + q) * 16 + col;
        koff[q] = 0;
        one[q] = k == d.K;
        if (k < d.K) {
            const int j = k % d.kf, gi = k / d.kf, i = gi % d.kt, g = gi / d.kt;
            koff[q] = i * d.rowW + g * d.Fp + j;
        }
    }
    for (int m = threadIdx.x; m < CF_TILE_M; m += CF_THREADS) {
        int o = 0;
        if (m < n_pos) {
            const int tl = m / d.F_out, f = m - tl * d.F_out;
            o = tl * d.st * d.rowW + f * d.sf;
        }
        posbase[m] = o;
    }
    f32x4 acc[4][NB];
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) acc[q][nb] = f32x4{0.f, 0.f, 0.f, 0.f};
    const bool wave_live = kb0 * 16 < k_rows;                        // (uniform per wave)
    for (int tile = blockIdx.x; tile < n_tiles; tile += n_part) {
        const int tt = tile / d.B, b = tile - tt * d.B;
        const int t0 = tt * d.tile_t;
        const int Lb = cf_row_len(lengths, b, d.T);
        const int Lo = (Lb + d.st - 1) / d.st;
        if (t0 >= Lo) continue;                                      // (uniform) nothing of this tile lies in the row
        __syncthreads();                                             // the previous tile has been read
        cf_stage_patch(d, x, b, t0, Lb, patch);
        for (int e = threadIdx.x; e < CF_TILE_M * d.C; e += CF_THREADS) {
            const int m = e / d.C, c = e - m * d.C;
            float v = 0.f;
            if (m < n_pos) {
                const int tl = m / d.F_out, f = m - tl * d.F_out;
                const int t = t0 + tl;
                if (t < Lo) {                                        // (Lo <= T_out) frames past the row are never read
                    const long at = ((long)t * d.B + b) * ystride + (long)f * d.C + c;
                    const float yv = y[at];
                    if (yv > 0.f && yv < 20.f) v = dy[at];
                }
            }
            gl[m * d.w_stride + c] = v;
        }
        __syncthreads();
        if (wave_live) {
            for (int s = 0; s < steps; ++s) {
                const int pos = s * 4 + kq;
                const int pb = posbase[pos];
                float a[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) a[q] = one[q] ? 1.f : patch[pb + koff[q]];
                const float* gr = gl + pos * d.w_stride + col;
#pragma unroll
                for (int nb = 0; nb < NB; ++nb) {
                    const float bv = gr[nb * 16];
#pragma unroll
                    for (int q = 0; q < 4; ++q) acc[q][nb] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[q], bv, acc[q][nb], 0, 0, 0);
                }
            }
        }
    }
    // part[p][row][c], rows 0 .. k_rows - 1 (k_rows = K + 1 rounded up to 16): written whether or not a tile was live
    float* tile_out = part + (long)blockIdx.x * k_rows * d.C;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = (kb0 + q) * 16 + kq * 4 + r;
            if (row >= k_rows) continue;
#pragma unroll
            for (int nb = 0; nb < NB; ++nb) tile_out[(long)row * d.C + nb * 16 + col] = acc[q][nb][r];
        }
    }
}

// out[e] += sum_p part[p][e], e < (K + 1) C: the first K C elements are dw, the last C are db.
__global__ __launch_bounds__(CF_SLICES * CF_RED_COLS) void conv2d_reduce_kernel(const float* __restrict__ part, int n_part, int per_slice,
                                                                                long part_stride, int n_dw, int n_elem,
                                                                                float* __restrict__ dw, float* __restrict__ db) {
    __shared__ float red[CF_SLICES][CF_RED_COLS];
    const int c = threadIdx.x % CF_RED_COLS, s = threadIdx.x / CF_RED_COLS;
    const int e = blockIdx.x * CF_RED_COLS + c;
    float acc = 0.f;
    if (e < n_elem) {
        const int p0 = s * per_slice;
        const int p1 = p0 + per_slice < n_part ? p0 + per_slice : n_part;
        for (int p = p0; p < p1; ++p) acc += part[(long)p * part_stride + e];
    }
    red[s][c] = acc;
    __syncthreads();
    if (s == 0 && e < n_elem) {
        float tot = red[0][c];
        for (int q = 1; q < CF_SLICES; ++q) tot += red[q][c];
        if (e < n_dw) dw[e] += tot;
        else db[e - n_dw] += tot;
    }
}

// ---- the plan: one function decides for every launch; amdspeech_conv2d_plan returns the same struct.  No device is needed.
static int plan_conv2d(int T, int B, int G, int F, int C, int kt, int kf, int st, int sf, CfDims* d, CfPlan* p) {
    AS_CHECK_ARG(T > 0 && B > 0, "conv2d: bad shape (T %d, B %d)", T, B);
    AS_CHECK_ARG(G >= 1 && G <= CF_MAX_G && F >= 1 && F <= CF_MAX_F, "conv2d: G %d outside 1 .. %d or F %d outside 1 .. %d", G, CF_MAX_G, F,
                 CF_MAX_F);
    AS_CHECK_ARG(C == 16 || C == 32 || C == 48 || C == 64, "conv2d: %d channels (16, 32, 48 or 64)", C);
    AS_CHECK_ARG(kt >= 1 && kt <= CF_MAX_KT && (kt & 1) && kf >= 1 && kf <= CF_MAX_KF && (kf & 1),
                 "conv2d: kernel %d x %d (both odd, time 1 .. %d, frequency 1 .. %d)", kt, kf, CF_MAX_KT, CF_MAX_KF);
    AS_CHECK_ARG(st >= 1 && st <= CF_MAX_STRIDE && sf >= 1 && sf <= CF_MAX_STRIDE, "conv2d: stride %d x %d (each 1 .. %d)", st, sf, CF_MAX_STRIDE);
    d->T = T; d->B = B; d->G = G; d->F = F; d->C = C; d->kt = kt; d->kf = kf; d->st = st; d->sf = sf;
    d->T_out = ceil_div(T, st);
    d->F_out = ceil_div(F, sf);
    AS_CHECK_ARG((long)d->F_out * C <= 4096, "conv2d: output width F' * C = %d * %d exceeds 4096", d->F_out, C);
    AS_CHECK_ARG((long)T * B * G * F < (1L << 31) && (long)d->T_out * B * d->F_out * C < (1L << 31),
                 "conv2d: shape too large (T %d, B %d, G %d, F %d, C %d)", T, B, G, F, C);
    d->K = G * kt * kf;
    d->k_pad = ceil_div(d->K, 4) * 4;
    d->pt = (kt - 1) / 2; d->pf = (kf - 1) / 2;
    d->Fp = F + 2 * d->pf;
    d->rowW = G * d->Fp;
    d->w_stride = cf_w_stride(C);
    // the tile: as many output frames as 128 positions hold, fewer where the patch would not fit beside the other LDS tenants of
    // EITHER pass (streamed weights forward, dy * mask backward).  It does not depend on T or B.
    const int fixed_fwd = d->k_pad * 4 + CF_K_STREAM * d->w_stride * 4;
    const int fixed_bwd = CF_TILE_M * 4 + CF_TILE_M * d->w_stride * 4;
    const int fixed = fixed_fwd > fixed_bwd ? fixed_fwd : fixed_bwd;
    int tile_t = CF_TILE_M / d->F_out;
    auto patch_bytes = [&](int tt) { return ((tt - 1) * st + kt) * d->rowW * 4; };
    while (tile_t > 1 && patch_bytes(tile_t) + fixed > CF_LDS_BUDGET) --tile_t;
    AS_CHECK_ARG(patch_bytes(tile_t) + fixed <= CF_LDS_BUDGET, "conv2d: one output frame's source span does not fit LDS (G %d, F %d, kernel %d x %d)",
                 G, F, kt, kf);
    d->tile_t = tile_t;
    d->span = (tile_t - 1) * st + kt;
    const int resident_bytes = patch_bytes(tile_t) + d->k_pad * 4 + d->k_pad * d->w_stride * 4;
    const bool resident = resident_bytes <= CF_LDS_BUDGET;
    d->k_chunk = resident ? d->k_pad : CF_K_STREAM;
    const int t_tiles = ceil_div(d->T_out, tile_t);
    AS_CHECK_ARG(B <= 65535, "conv2d: B %d exceeds 65535", B);
    if (p) {
        p->t_out = d->T_out; p->f_out = d->F_out; p->k = d->K; p->k_pad = d->k_pad;
        p->tile_t = tile_t; p->tile_f = d->F_out; p->vec = 1;
        p->fwd_workgroups = t_tiles * B;
        p->fwd_lds_bytes = resident ? resident_bytes : patch_bytes(tile_t) + fixed_fwd;
        p->weights_resident = resident ? 1 : 0;
        p->k_chunk = d->k_chunk;
        p->k_rows = ceil_div(d->K + 1, 16) * 16;
        p->k_groups = ceil_div(p->k_rows, CF_KROWS_WG);
        const int n_tiles = t_tiles * B;
        const int want = ceil_div(CF_DW_TARGET_WGS, p->k_groups);
        p->dw_partials = n_tiles < want ? n_tiles : want;
        p->bwd_workgroups = p->dw_partials * p->k_groups;
        p->bwd_lds_bytes = patch_bytes(tile_t) + fixed_bwd;
        p->dw_terms = ceil_div(n_tiles, p->dw_partials) * tile_t * d->F_out;
        p->reduce_slices = CF_SLICES;
        p->reduce_terms = ceil_div(p->dw_partials, CF_SLICES);
        p->reduce_workgroups = ceil_div((long)(d->K + 1) * C, CF_RED_COLS);
    }
    return AMDSPEECH_OK;
}

// dw_partials grows with T and is capped by a figure that does not depend on it: the bytes cover every shorter T.
static size_t conv2d_ws_bytes(const CfPlan& p, int C) { return (size_t)p.dw_partials * (size_t)p.k_rows * (size_t)C * sizeof(float); }

static bool cf_overlap(const void* a, size_t na, const void* b, size_t nb) {
    const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
    return !(x + na <= y || y + nb <= x);
}

static int run_conv2d_fwd(hipStream_t s, const float* x, const float* w, const float* bias, const int* lengths, int T, int B, int G, int F,
                          int C, int kt, int kf, int st, int sf, float* y, int* lengths_out) {
    AS_CHECK_ARG(x && w && bias && lengths && y && lengths_out, "conv2d_fwd: null pointer");
    CfDims d;
    CfPlan pl;
    if (int rc = plan_conv2d(T, B, G, F, C, kt, kf, st, sf, &d, &pl)) return rc;
    AS_CHECK_ARG(!cf_overlap(x, (size_t)T * B * G * F * 4, y, (size_t)d.T_out * B * d.F_out * C * 4), "conv2d_fwd: x and y overlap");
    const dim3 grid(ceil_div(d.T_out, d.tile_t), B), block(CF_THREADS);
    switch (C / 16) {
    case 1: hipLaunchKernelGGL(conv2d_fwd_kernel<1>, grid, block, pl.fwd_lds_bytes, s, d, x, w, bias, lengths, y, lengths_out); break;
    case 2: hipLaunchKernelGGL(conv2d_fwd_kernel<2>, grid, block, pl.fwd_lds_bytes, s, d, x, w, bias, lengths, y, lengths_out); break;
    case 3: hipLaunchKernelGGL(conv2d_fwd_kernel<3>, grid, block, pl.fwd_lds_bytes, s, d, x, w, bias, lengths, y, lengths_out); break;
    default: hipLaunchKernelGGL(conv2d_fwd_kernel<4>, grid, block, pl.fwd_lds_bytes, s, d, x, w, bias, lengths, y, lengths_out); break;
    }
    AS_CHECK_LAUNCH();
    return AMDSPEECH_OK;
}

static int run_conv2d_bwd(hipStream_t s, const float* x, const float* y, const float* dy, const int* lengths, int T, int B, int G, int F,
                          int C, int kt, int kf, int st, int sf, float* dw, float* db, void* ws) {
    AS_CHECK_ARG(x && y && dy && lengths && dw && db && ws, "conv2d_bwd: null pointer");
    AS_CHECK_ARG((reinterpret_cast<uintptr_t>(ws) & 3) == 0, "conv2d_bwd: the workspace must be 4-byte aligned");
    CfDims d;
    CfPlan pl;
    if (int rc = plan_conv2d(T, B, G, F, C, kt, kf, st, sf, &d, &pl)) return rc;
    const size_t wbytes = (size_t)d.K * C * 4, pbytes = conv2d_ws_bytes(pl, C);
    AS_CHECK_ARG(!cf_overlap(dw, wbytes, ws, pbytes) && !cf_overlap(db, (size_t)C * 4, ws, pbytes) && !cf_overlap(dw, wbytes, db, (size_t)C * 4),
                 "conv2d_bwd: dw, db and the workspace overlap");
    float* part = static_cast<float*>(ws);
    const dim3 grid(pl.dw_partials, pl.k_groups), block(CF_THREADS);
    const int n_tiles = ceil_div(d.T_out, d.tile_t) * B;
    switch (C / 16) {
    case 1: hipLaunchKernelGGL(conv2d_dw_kernel<1>, grid, block, pl.bwd_lds_bytes, s, d, x, y, dy, lengths, n_tiles, pl.dw_partials, pl.k_rows, part); break;
    case 2: hipLaunchKernelGGL(conv2d_dw_kernel<2>, grid, block, pl.bwd_lds_bytes, s, d, x, y, dy, lengths, n_tiles, pl.dw_partials, pl.k_rows, part); break;
    case 3: hipLaunchKernelGGL(conv2d_dw_kernel<3>, grid, block, pl.bwd_lds_bytes, s, d, x, y, dy, lengths, n_tiles, pl.dw_partials, pl.k_rows, part); break;
    default: hipLaunchKernelGGL(conv2d_dw_kernel<4>, grid, block, pl.bwd_lds_bytes, s, d, x, y, dy, lengths, n_tiles, pl.dw_partials, pl.k_rows, part); break;
    }
    AS_CHECK_LAUNCH();
    hipLaunchKernelGGL(conv2d_reduce_kernel, dim3(pl.reduce_workgroups), dim3(CF_SLICES * CF_RED_COLS), 0, s, part, pl.dw_partials,
                       pl.reduce_terms, (long)pl.k_rows * C, d.K * C, (d.K + 1) * C, dw, db);
    AS_CHECK_LAUNCH();
    return AMDSPEECH_OK;
}

}  // namespace amdspeech

using namespace amdspeech;

extern "C" int amdspeech_conv2d_plan(int T, int B, int G, int F, int C, int kt, int kf, int st, int sf, amdspeech_conv2d_plan_info* out) {
    AS_CHECK_ARG(out != nullptr, "conv2d_plan: null output");
    CfDims d;
    return plan_conv2d(T, B, G, F, C, kt, kf, st, sf, &d, out);
}

extern "C" size_t amdspeech_conv2d_bwd_workspace_bytes(int T, int B, int G, int F, int C, int kt, int kf, int st, int sf) {
    CfDims d;
    CfPlan pl;
    if (plan_conv2d(T, B, G, F, C, kt, kf, st, sf, &d, &pl) != AMDSPEECH_OK) return 0;
    return conv2d_ws_bytes(pl, C);
}

extern "C" int amdspeech_conv2d_fwd(void* stream, const float* x, const float* w, const float* bias, const int* lengths, int T, int B, int G,
                                    int F, int C, int kt, int kf, int st, int sf, float* y, int* lengths_out) {
    return run_conv2d_fwd(static_cast<hipStream_t>(stream), x, w, bias, lengths, T, B, G, F, C, kt, kf, st, sf, y, lengths_out);
}

extern "C" int amdspeech_conv2d_bwd(void* stream, const float* x, const float* y, const float* dy, const int* lengths, int T, int B, int G,
                                    int F, int C, int kt, int kf, int st, int sf, float* dw, float* db, void* ws) {
    return run_conv2d_bwd(static_cast<hipStream_t>(stream), x, y, dy, lengths, T, B, G, F, C, kt, kf, st, sf, dw, db, ws);
}
