// The transducer (RNN-T) objective (amdspeech.h: "transducer"): label preparation, the joint network in both
// directions, and the lattice loss with its gradient.  No reference counterpart: the reference trains with CTC only.
//
// Regime.  The lattice has N = B T (U+1) nodes (1.73 M at the headline shape), every node a row of the joint: z = tanh(f_t + g_u),
// logits = z . W_out + b_out with J 512 and C 80.  z at N x J floats is gigabytes, so it only ever exists as MFMA operands:
//   joint_fwd   a workgroup owns one utterance, 4 frames (one per wave) and 16 MT prefix positions.  W_out, the g strip and the f
//               strip pass through LDS in chunks of 32 k; a lane forms its A operands tanh(f + g) in registers and feeds
//               v_mfma_f32_16x16x4_f32 with the nodes on the A port.  The k order of a node's sum is a function of J alone.
//   loss        the lattice recursions in float64 by anti-diagonals, one workgroup per (utterance, direction), alpha and beta
//               concurrently (the latency regime of ctc.hip: a barrier per diagonal); the blank and label log-probabilities of
//               every live node are gathered by a row kernel first, the gradient is a second row kernel that re-reads the row.
//   joint_bwd   a workgroup owns one utterance, a chunk of frames and a slice of J.  Per 16 nodes: dlogits . W_out^T on the MFMA
//               with the nodes on the A port, z recomputed in the accumulator layout, dz = (.) (1 - z^2); the SAME z registers are
//               the A operand of z^T . dlogits (nodes now the contraction).  df is summed over u in LDS (the workgroup sees every
//               u of its frames) and written directly, dg over the chunk's frames in registers and left as one partial per chunk,
//               dW_out / db_out as one partial per workgroup; two small kernels add the partials in a fixed order.
// No floating-point atomics anywhere; every offset into a lattice tensor is size_t.
#include "common.h"

#include <math.h>

namespace amdspeech {

constexpr int RT_THREADS = 256;
constexpr int RT_J_MAX = 1024;
constexpr int RT_C_MAX = 256;
constexpr int RT_U_MAX = 2559;
constexpr int RT_KC = 32;                      // joint_fwd: k per LDS chunk
constexpr int RT_LDG = RT_KC + 4;              // ... pitch of the g strip in LDS (rows 36 words apart: the 16 x 4 lanes of a fragment hit 64 banks)
constexpr int RT_BWD_MT = 1;                   // joint_bwd: 16-node sub-tiles per wave
constexpr int RT_TC_MIN = 32, RT_TC_MAX = 128; // joint_bwd: frames per chunk
constexpr int RT_CHUNKS = 8;                   // ... chunks aimed at (T <= 8 RT_TC_MAX)

typedef amdspeech_rnnt_plan_info RnntPlan;

// The instantiation of a class count: column tiles of 16 (joint_fwd and joint_bwd), node sub-tiles per wave (joint_fwd) and
// k tiles of 16 per J slice (joint_bwd).  The accumulators of a wave are MT x NT (forward) and KT x NT (dW_out) tiles of 4 registers.
struct ColClass { int c_min, c_max, nt, mt, kt; };
static const ColClass RT_CLASSES[4] = {{2, 32, 2, 4, 4}, {33, 80, 5, 4, 4}, {81, 128, 8, 2, 2}, {129, 256, 16, 1, 1}};

struct RecClass { int kernel, u_min, u_max, threads, states; };      // U + 1 lattice columns over threads x states
static const RecClass RT_REC[4] = {{AMDSPEECH_RNNT_REC_WAVE, 1, 63, 64, 1},
                                   {AMDSPEECH_RNNT_REC_BLOCK1, 64, 255, 256, 1},
                                   {AMDSPEECH_RNNT_REC_BLOCK4, 256, 1023, 256, 4},
                                   {AMDSPEECH_RNNT_REC_BLOCK10, 1024, RT_U_MAX, 256, 10}};

static int fwd_ldw(int nt) { return nt * 16 + ((16 - (nt * 16) % 64) + 64) % 64; }      // pitch = 16 mod 64 words: k rows 16 banks apart

static int plan_rnnt(int T, int B, int U, int J, int C, RnntPlan* p) {
    AS_CHECK_ARG(T >= 1 && B >= 1, "rnnt: T = %d and B = %d must be positive", T, B);
    AS_CHECK_ARG(J >= 16 && J % 16 == 0, "rnnt: J = %d must be a positive multiple of 16", J);
    AS_CHECK_ARG(C >= 2, "rnnt: C = %d must be at least 2", C);
    AS_CHECK_ARG(U >= 1, "rnnt: U = %d must be at least 1", U);
    if (J > RT_J_MAX) { set_error("rnnt: J = %d above the kernels' limit of %d", J, RT_J_MAX); return AMDSPEECH_EUNSUPPORTED; }
    if (C > RT_C_MAX) { set_error("rnnt: C = %d above the kernels' limit of %d", C, RT_C_MAX); return AMDSPEECH_EUNSUPPORTED; }
    if (U > RT_U_MAX) { set_error("rnnt: U = %d above the kernels' limit of %d", U, RT_U_MAX); return AMDSPEECH_EUNSUPPORTED; }
    const long long N = (long long)B * T * (U + 1);
    if (N * C >= (1LL << 31)) {
        set_error("rnnt: B * T * (U + 1) * C = %lld must be below 2^31", N * C);
        return AMDSPEECH_EUNSUPPORTED;
    }
    const ColClass* cc = &RT_CLASSES[0];
    for (int i = 0; i < 4; ++i)
        if (C >= RT_CLASSES[i].c_min && C <= RT_CLASSES[i].c_max) cc = &RT_CLASSES[i];
    const RecClass* rc = &RT_REC[0];
    for (int i = 0; i < 4; ++i)
        if (U >= RT_REC[i].u_min && U <= RT_REC[i].u_max) rc = &RT_REC[i];
    *p = RnntPlan();
    p->threads = RT_THREADS;
    p->col_tiles = cc->nt; p->c_min = cc->c_min; p->c_max = cc->c_max;
    p->j_min = 16; p->j_max = RT_J_MAX;
    p->fwd_t_tile = 4; p->fwd_u_tile = 16 * cc->mt; p->fwd_k_chunk = RT_KC;
    p->fwd_t_tiles = ceil_div(T, 4); p->fwd_u_tiles = ceil_div(U + 1, p->fwd_u_tile);
    p->fwd_grid = p->fwd_t_tiles * p->fwd_u_tiles * B;      // (below N: fits)
    p->fwd_lds_bytes = (RT_KC * fwd_ldw(cc->nt) + 16 * cc->mt * RT_LDG + 4 * RT_KC) * 4;
    p->rows_per_workgroup = RT_THREADS / 64;
    p->rows_grid = ceil_div(N, p->rows_per_workgroup);
    p->rec_kernel = rc->kernel; p->rec_threads = rc->threads; p->rec_states = rc->states;
    p->u_min = rc->u_min; p->u_max = rc->u_max;
    p->rec_grid = 2 * B;
    p->rec_lds_bytes = 2 * rc->threads * rc->states * 8;
    p->bwd_t_tile = 4; p->bwd_u_tile = 16 * RT_BWD_MT;
    p->bwd_k_slice = 16 * cc->kt; p->bwd_k_slices = ceil_div(J, p->bwd_k_slice);
    int tc = ceil_div(ceil_div(T, RT_CHUNKS), 4) * 4;
    tc = tc < RT_TC_MIN ? RT_TC_MIN : (tc > RT_TC_MAX ? RT_TC_MAX : tc);
    p->bwd_t_chunk = tc; p->bwd_t_chunks = ceil_div(T, tc);
    p->bwd_items = B * p->bwd_t_chunks;
    p->bwd_grid = p->bwd_items * p->bwd_k_slices;
    p->bwd_lds_bytes = (p->bwd_k_slice * (cc->nt * 16 + 1) + RT_TC_MAX * p->bwd_k_slice + 4 * 256) * 4;
    p->dg_terms = p->bwd_t_chunks; p->dw_terms = p->bwd_items;
    p->reduce_dg_grid = ceil_div((long)(U + 1) * B * J, RT_THREADS);
    p->reduce_dw_grid = ceil_div((long)J * C + C, RT_THREADS);
    p->launches_fwd = 1; p->launches_loss = 3; p->launches_bwd = 3;
    return AMDSPEECH_OK;
}

// workspace regions, each rounded up to 256 bytes (amdspeech.h documents the sum)
struct RnntWs { size_t lpb, lpy, alpha, beta, lnp, dgp, dwp, dbp, total; };
static RnntWs ws_layout(int T, int B, int U, int J, int C, const RnntPlan& p) {
    const size_t N = (size_t)B * T * (U + 1);
    RnntWs w;
    size_t o = 0;
    w.lpb = o; o += align_up(N * 4, 256);
    w.lpy = o; o += align_up(N * 4, 256);
    w.alpha = o; o += align_up(N * 8, 256);
    w.beta = o; o += align_up(N * 8, 256);
    w.lnp = o; o += align_up((size_t)B * 8, 256);
    w.dgp = o; o += align_up((size_t)p.bwd_t_chunks * (U + 1) * B * J * 4, 256);
    w.dwp = o; o += align_up((size_t)p.bwd_items * J * C * 4, 256);
    w.dbp = o; o += align_up((size_t)p.bwd_items * C * 4, 256);
    w.total = o;
    return w;
}

__device__ __forceinline__ int rt_clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// ---------------------------------------------------------------------------------------------------------------- targets
// One wave per row: the sparsification of ctc_prepare_kernel (zeros dropped, the target is every kept label before the first
// one >= C-1), without its empty-row and required-time rules.  Negative ids are dropped with the zeros, so every target is a class
// in 1 .. C-2 and ln P of a live row is finite.
__global__ __launch_bounds__(64) void rnnt_targets_kernel(const int* __restrict__ dense, int U, int C, int* __restrict__ targets,
                                                          int* __restrict__ n, int* __restrict__ tok, int* __restrict__ tok_len) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const int blank = C - 1;
    int* tg = targets + (size_t)b * U;
    int* tk = tok + (size_t)b * (U + 2);
    for (int s = lane; s < U; s += 64) tg[s] = 0;
    for (int s = lane; s < U + 2; s += 64) tk[s] = blank;
    __syncthreads();
    int ntgt = 0;
    const unsigned long long lt = (1ull << lane) - 1ull;
    for (int u0 = 0; u0 < U; u0 += 64) {
        const int u = u0 + lane;
        const int v = (u < U) ? dense[(size_t)b * U + u] : 0;
        const bool nz = v > 0;                                    // (0 is the padding; a negative id is no label either: dropped)
        const unsigned long long mnz = __ballot(nz);
        const unsigned long long mterm = __ballot(nz && v >= blank);
        unsigned long long before = ~0ull;
        if (mterm) before = (1ull << (__ffsll((long long)mterm) - 1)) - 1ull;
        const unsigned long long mt = mnz & before;               // targets in this chunk
        if (nz && ((mt >> lane) & 1ull)) {
            const int pos = ntgt + __popcll(mt & lt);
            tg[pos] = v;
            tk[pos + 1] = v;
        }
        ntgt += __popcll(mt);
        if (mterm) break;                                         // (uniform over the wave)
    }
    if (lane == 0) {
        n[b] = ntgt;
        tok_len[b] = ntgt + 1;
    }
}

// ---------------------------------------------------------------------------------------------------------------- joint, forward
struct JointArgs {
    int T, B, U, J, C;
    int t_tiles, u_tiles;
    const float *f, *g, *w, *bias;
    const int *lengths, *n;
    float* logits;
};

template <int MT, int NT>
__global__ __launch_bounds__(RT_THREADS) void rnnt_joint_fwd_kernel(JointArgs a) {
    constexpr int CP = NT * 16;
    constexpr int LDW = CP + ((16 - CP % 64) + 64) % 64;
    __shared__ float Wl[RT_KC][LDW];
    __shared__ float gl[16 * MT][RT_LDG];
    __shared__ float fl[4][RT_KC];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int li = lane & 15, lg = lane >> 4;
    const int T = a.T, B = a.B, U1 = a.U + 1, J = a.J, C = a.C;
    int item = blockIdx.x;
    const int ut = item % a.u_tiles; item /= a.u_tiles;
    const int tt = item % a.t_tiles;
    const int b = item / a.t_tiles;
    if (b >= B) return;
    const int Tb = rt_clampi(a.lengths[b], 0, T), nb = rt_clampi(a.n[b], 0, a.U);
    const int t0 = tt * 4, u0 = ut * (16 * MT);
    if (t0 >= Tb || u0 > nb) return;                              // (uniform over the workgroup: no live node in the tile)
    const int t = t0 + wave;
    const f32x4 zero4 = {0.0f, 0.0f, 0.0f, 0.0f};
    f32x4 acc[MT][NT];
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int q = 0; q < NT; ++q) acc[m][q] = zero4;

    for (int k0 = 0; k0 < J; k0 += RT_KC) {
        const int kc = J - k0 < RT_KC ? J - k0 : RT_KC;           // 32, or 16 at the end of a J that is no multiple of 32
        __syncthreads();                                          // (the previous chunk has been consumed)
        for (int e = tid; e < RT_KC * CP; e += RT_THREADS) {
            const int kk = e / CP, c = e % CP;
            Wl[kk][c] = (kk < kc && c < C) ? a.w[(size_t)(k0 + kk) * C + c] : 0.0f;
        }
        for (int e = tid; e < 16 * MT * RT_KC; e += RT_THREADS) {
            const int r = e / RT_KC, kk = e % RT_KC;
            const int u = u0 + r;
            gl[r][kk] = (kk < kc && u < U1) ? a.g[((size_t)u * B + b) * J + k0 + kk] : 0.0f;
        }
        if (tid < 4 * RT_KC) {
            const int r = tid / RT_KC, kk = tid % RT_KC;
            fl[r][kk] = (kk < kc && t0 + r < T) ? a.f[((size_t)(t0 + r) * B + b) * J + k0 + kk] : 0.0f;
        }
        __syncthreads();
        for (int kb = 0; kb < kc; kb += 16) {
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const int kk = kb + lg + 4 * s;                   // this lane's k of MFMA s: the four lane groups interleaved
                const float fv = fl[wave][kk];
                float av[MT], bv[NT];
#pragma unroll
                for (int m = 0; m < MT; ++m) av[m] = tanhf(fv + gl[16 * m + li][kk]);
#pragma unroll
                for (int q = 0; q < NT; ++q) bv[q] = Wl[kk][q * 16 + li];
#pragma unroll
                for (int m = 0; m < MT; ++m)
#pragma unroll
                    for (int q = 0; q < NT; ++q) acc[m][q] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[m], bv[q], acc[m][q], 0, 0, 0);
            }
        }
    }
    if (t >= Tb) return;                                          // (after the last barrier)
    // D[i][j] of a tile: lane (i / 4) * 16 + j, register i % 4
    const size_t row_t = ((size_t)b * T + t) * U1;
#pragma unroll
    for (int q = 0; q < NT; ++q) {
        const int c = q * 16 + li;
        if (c >= C) continue;
        const float bias = a.bias[c];
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int u = u0 + 16 * m + 4 * lg + r;
                if (u <= nb) a.logits[(row_t + u) * C + c] = acc[m][q][r] + bias;
            }
    }
}

// ---------------------------------------------------------------------------------------------------------------- loss
struct LossArgs {
    int T, B, U, C;
    const float* logits;
    const int *targets, *n, *lengths;
    float *lpb, *lpy;
    double *alpha, *beta, *lnp;
    float *loss, *dlogits;
};

// a row's maximum and log of the sum in float32, the lanes meeting in a 32-16-8-4-2-1 xor butterfly: a fixed function of C
__device__ __forceinline__ void rt_row_stats(const float (&x)[4], int lane, int C, float& mx, float& logs) {
    float m = -INFINITY;
#pragma unroll
    for (int q = 0; q < 4; ++q) m = fmaxf(m, x[q]);
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
    float s = 0.0f;
#pragma unroll
    for (int q = 0; q < 4; ++q) s += lane + 64 * q < C ? expf(x[q] - m) : 0.0f;
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    mx = m;
    logs = logf(s);
}

// one wave per lattice node: the blank and the label log-probability of every live node
__global__ __launch_bounds__(RT_THREADS) void rnnt_rows_kernel(LossArgs a) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63;
    const size_t U1 = (size_t)a.U + 1;
    const size_t N = (size_t)a.B * a.T * U1;
    const size_t i = (size_t)blockIdx.x * (RT_THREADS / 64) + (threadIdx.x >> 6);
    if (i >= N) return;
    const int u = (int)(i % U1);
    const int t = (int)((i / U1) % a.T);
    const int b = (int)(i / (U1 * a.T));
    const int Tb = rt_clampi(a.lengths[b], 0, a.T), nb = rt_clampi(a.n[b], 0, a.U);
    if (t >= Tb || u > nb) return;
    const int C = a.C;
    const float* row = a.logits + i * C;
    float x[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) x[q] = lane + 64 * q < C ? row[lane + 64 * q] : -INFINITY;
    float m, logs;
    rt_row_stats(x, lane, C, m, logs);
    int y = -1;
    if (u < nb) y = a.targets[(size_t)b * a.U + u];
    if (u < nb && (y < 0 || y >= C) && lane == 0) a.lpy[i] = -INFINITY;      // (a label outside the classes: no such path)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int c = lane + 64 * q;
        const float lp = (x[q] - m) - logs;
        if (c == C - 1) a.lpb[i] = lp;
        if (c == y) a.lpy[i] = lp;
    }
}

__device__ __forceinline__ double rt_logaddexp(double p, double q) {
    const double hi = p > q ? p : q, lo = p > q ? q : p;
    if (hi == -INFINITY) return hi;
    return hi + log1p(exp(lo - hi));
}

// alpha (blockIdx.x even) and beta (odd) of one utterance by anti-diagonals; column u of the lattice lives in thread u % THREADS,
// the previous diagonal in LDS (two buffers, one barrier per diagonal).  The log-probabilities of the NEXT diagonal are loaded
// before the barrier of this one.
template <int THREADS, int R>
__global__ __launch_bounds__(THREADS) void rnnt_lattice_kernel(LossArgs a) {
    __shared__ double buf[2][THREADS * R];
    const int tid = threadIdx.x;
    const int b = blockIdx.x >> 1, dir = blockIdx.x & 1;
    const int T = a.T, U1 = a.U + 1;
    const int Tb = rt_clampi(a.lengths[b], 0, T), nb = rt_clampi(a.n[b], 0, a.U);
    if (Tb == 0) {
        if (dir == 0 && tid == 0) { a.loss[b] = 0.0f; a.lnp[b] = 0.0; }
        return;
    }
    const size_t base = (size_t)b * T * U1;
    const int last = Tb - 1 + nb;
    const double ninf = -INFINITY;
    for (int r = 0; r < R; ++r) { buf[0][tid + THREADS * r] = ninf; buf[1][tid + THREADS * r] = ninf; }
    __syncthreads();
    // the two log-probabilities a column needs on diagonal d: alpha reads blank at (t-1, u) and label at (t, u-1), beta both at (t, u)
    auto fetch = [&](int d, float (&vb)[R], float (&vy)[R]) {
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int u = tid + THREADS * r, t = d - u;
            vb[r] = 0.0f; vy[r] = 0.0f;
            if (d < 0 || d > last || u > nb || t < 0 || t >= Tb) continue;
            if (dir == 0) {
                if (t > 0) vb[r] = a.lpb[base + (size_t)(t - 1) * U1 + u];
                if (u > 0) vy[r] = a.lpy[base + (size_t)t * U1 + u - 1];
            } else {
                vb[r] = a.lpb[base + (size_t)t * U1 + u];
                if (u < nb) vy[r] = a.lpy[base + (size_t)t * U1 + u];
            }
        }
    };
    float vb[R], vy[R], nvb[R], nvy[R];
    const int step = dir == 0 ? 1 : -1;
    int d = dir == 0 ? 0 : last;
    fetch(d, vb, vy);
    int cur = 0;
    for (int it = 0; it <= last; ++it, d += step) {
        fetch(d + step, nvb, nvy);
        const double* prev = buf[cur ^ 1];
        double* now = buf[cur];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int u = tid + THREADS * r, t = d - u;
            if (u > nb || t < 0 || t >= Tb) continue;
            double v;
            if (dir == 0) {
                if (d == 0) v = 0.0;
                else {
                    const double p1 = t > 0 ? prev[u] + (double)vb[r] : ninf;
                    const double p2 = u > 0 ? prev[u - 1] + (double)vy[r] : ninf;
                    v = rt_logaddexp(p1, p2);
                }
                a.alpha[base + (size_t)t * U1 + u] = v;
            } else {
                if (d == last) v = (double)vb[r];
                else {
                    const double p1 = t + 1 < Tb ? prev[u] + (double)vb[r] : ninf;
                    const double p2 = u < nb ? prev[u + 1] + (double)vy[r] : ninf;
                    v = rt_logaddexp(p1, p2);
                }
                a.beta[base + (size_t)t * U1 + u] = v;
            }
            now[u] = v;
        }
#pragma unroll
        for (int r = 0; r < R; ++r) { vb[r] = nvb[r]; vy[r] = nvy[r]; }
        __syncthreads();
        cur ^= 1;
    }
    if (dir == 0 && tid == 0) {
        const double lnp = buf[cur ^ 1][nb] + (double)a.lpb[base + (size_t)(Tb - 1) * U1 + nb];
        a.lnp[b] = lnp;
        a.loss[b] = (float)(-lnp);
    }
}

// one wave per lattice node: the gradient row.  The row is in registers before anything is written (dlogits may be logits).
__global__ __launch_bounds__(RT_THREADS) void rnnt_grad_kernel(LossArgs a) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63;
    const size_t U1 = (size_t)a.U + 1;
    const size_t N = (size_t)a.B * a.T * U1;
    const size_t i = (size_t)blockIdx.x * (RT_THREADS / 64) + (threadIdx.x >> 6);
    if (i >= N) return;
    const int u = (int)(i % U1);
    const int t = (int)((i / U1) % a.T);
    const int b = (int)(i / (U1 * a.T));
    const int Tb = rt_clampi(a.lengths[b], 0, a.T), nb = rt_clampi(a.n[b], 0, a.U);
    const int C = a.C;
    float* out = a.dlogits + i * C;
    if (t >= Tb || u > nb) {
#pragma unroll
        for (int q = 0; q < 4; ++q)
            if (lane + 64 * q < C) out[lane + 64 * q] = 0.0f;
        return;
    }
    const float* row = a.logits + i * C;
    float x[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) x[q] = lane + 64 * q < C ? row[lane + 64 * q] : -INFINITY;
    float m, logs;
    rt_row_stats(x, lane, C, m, logs);
    // lane 0: gamma, lane 1: the blank term, lane 2: the label term, each in float64 and rounded once
    const double al = a.alpha[i], lnp = a.lnp[b];
    float term = 0.0f;
    if (lane == 0) term = (float)exp(al + a.beta[i] - lnp);
    if (lane == 1) {
        double bn = -INFINITY;
        if (t + 1 < Tb) bn = a.beta[i + U1];
        else if (u == nb) bn = 0.0;                               // beta past the terminal node
        term = (float)exp(al + (double)a.lpb[i] + bn - lnp);
    }
    if (lane == 2 && u < nb) term = (float)exp(al + (double)a.lpy[i] + a.beta[i + 1] - lnp);
    const float gam = __shfl(term, 0, 64), eb = __shfl(term, 1, 64), ey = __shfl(term, 2, 64);
    int y = -1;
    if (u < nb) y = a.targets[(size_t)b * a.U + u];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int c = lane + 64 * q;
        if (c >= C) continue;
        float d = expf((x[q] - m) - logs) * gam;
        if (c == C - 1) d -= eb;
        if (c == y) d -= ey;
        out[c] = d;
    }
}

// ---------------------------------------------------------------------------------------------------------------- joint, backward
struct BwdArgs {
    int T, B, U, J, C;
    int tc, t_chunks;
    const float *dl, *f, *g, *w;
    const int *lengths, *n;
    float *df, *dgp, *dwp, *dbp;
    float *dg, *dw, *db;
    int items;
};

template <int NT, int KT>
__global__ __launch_bounds__(RT_THREADS) void rnnt_joint_bwd_kernel(BwdArgs a) {
    constexpr int CP = NT * 16, LDW = CP + 1, KS = KT * 16, MT = RT_BWD_MT;
    __shared__ float Wl[KS][LDW];
    __shared__ float dfl[RT_TC_MAX][KS];
    __shared__ __attribute__((aligned(16))) float red[4][256];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int li = lane & 15, lg = lane >> 4;
    const int T = a.T, B = a.B, U = a.U, U1 = a.U + 1, J = a.J, C = a.C;
    const int item = blockIdx.x;
    const int chunk = item % a.t_chunks, b = item / a.t_chunks;
    const int ks0 = blockIdx.y * KS;
    const int ktn = (J - ks0) / 16 < KT ? (J - ks0) / 16 : KT;      // k tiles of the slice inside J
    const int Tb = rt_clampi(a.lengths[b], 0, T), nb = rt_clampi(a.n[b], 0, U);
    const int tc0 = chunk * a.tc;
    const int tc1 = tc0 + a.tc < T ? tc0 + a.tc : T;
    const int tlive = tc1 < Tb ? tc1 : Tb;                          // frames tc0 .. tlive-1 have live nodes
    const f32x4 zero4 = {0.0f, 0.0f, 0.0f, 0.0f};

    for (int e = tid; e < RT_TC_MAX * KS; e += RT_THREADS) dfl[e / KS][e % KS] = 0.0f;
    for (int e = tid; e < KS * CP; e += RT_THREADS) {
        const int kk = e / CP, c = e % CP;
        Wl[kk][c] = (ks0 + kk < J && c < C) ? a.w[(size_t)(ks0 + kk) * C + c] : 0.0f;
    }
    __syncthreads();

    f32x4 accW[KT][NT];
    float dbacc[NT];
#pragma unroll
    for (int kt = 0; kt < KT; ++kt)
#pragma unroll
        for (int q = 0; q < NT; ++q) accW[kt][q] = zero4;
#pragma unroll
    for (int q = 0; q < NT; ++q) dbacc[q] = 0.0f;

    if (tc0 < tlive) {
        for (int u0 = 0; u0 <= nb; u0 += 16 * MT) {
            f32x4 dgacc[MT][KT];
#pragma unroll
            for (int m = 0; m < MT; ++m)
#pragma unroll
                for (int kt = 0; kt < KT; ++kt) dgacc[m][kt] = zero4;
            for (int t0 = tc0; t0 < tlive; t0 += 4) {
                const int t = t0 + wave;
                if (t >= tlive) continue;                          // (uniform over the wave; no barrier inside this loop)
                const size_t row_t = ((size_t)b * T + t) * U1;
#pragma unroll
                for (int m = 0; m < MT; ++m) {
                    const int ub = u0 + 16 * m;
                    if (ub > nb) continue;                         // (uniform)
                    // dlogits . W_out^T: the nodes on the A port, c the contraction
                    f32x4 acc[KT];
#pragma unroll
                    for (int kt = 0; kt < KT; ++kt) acc[kt] = zero4;
                    {
                        const int ua = ub + li;
                        const bool oka = ua <= nb;
                        const float* pa = a.dl + (row_t + (oka ? ua : nb)) * C;
                        for (int c0 = 0; c0 < CP; c0 += 16) {
#pragma unroll
                            for (int s = 0; s < 4; ++s) {
                                const int c = c0 + 4 * lg + s;
                                const float v = pa[c < C ? c : 0];
                                const float av = (oka && c < C) ? v : 0.0f;
#pragma unroll
                                for (int kt = 0; kt < KT; ++kt)
                                    acc[kt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, Wl[kt * 16 + li][c], acc[kt], 0, 0, 0);
                            }
                        }
                    }
                    // z in the accumulator layout (node 4 lg + r, k = li), dz, and what it sums to
                    float zz[KT][4];
#pragma unroll
                    for (int kt = 0; kt < KT; ++kt) {
                        const bool kok = kt < ktn;
                        const int k = ks0 + kt * 16 + li;
                        const float fv = kok ? a.f[((size_t)t * B + b) * J + k] : 0.0f;
                        float sdf = 0.0f;
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const int u = ub + 4 * lg + r;
                            const bool ok = kok && u <= nb;
                            const float gv = ok ? a.g[((size_t)u * B + b) * J + k] : 0.0f;
                            const float z = tanhf(fv + gv);
                            zz[kt][r] = ok ? z : 0.0f;
                            const float dz = ok ? acc[kt][r] * (1.0f - z * z) : 0.0f;
                            dgacc[m][kt][r] += dz;
                            sdf += dz;
                        }
                        sdf += __shfl_xor(sdf, 16, 64);
                        sdf += __shfl_xor(sdf, 32, 64);
                        if (lg == 0 && kok) dfl[t - tc0][kt * 16 + li] += sdf;      // (frame t belongs to this wave alone)
                    }
                    // z^T . dlogits: k on the A port, the nodes the contraction
#pragma unroll
                    for (int s = 0; s < 4; ++s) {
                        const int u = ub + 4 * lg + s;
                        const bool ok = u <= nb;
                        const float* pb = a.dl + (row_t + (ok ? u : nb)) * C;
                        float bv[NT];
#pragma unroll
                        for (int q = 0; q < NT; ++q) {
                            const int c = q * 16 + li;
                            const float v = pb[c < C ? c : 0];
                            bv[q] = (ok && c < C) ? v : 0.0f;
                            dbacc[q] += bv[q];
                        }
#pragma unroll
                        for (int kt = 0; kt < KT; ++kt)
#pragma unroll
                            for (int q = 0; q < NT; ++q)
                                accW[kt][q] = __builtin_amdgcn_mfma_f32_16x16x4f32(zz[kt][s], bv[q], accW[kt][q], 0, 0, 0);
                    }
                }
            }
            // dg of this u tile over the chunk's frames: the four waves in wave order, one partial per chunk
#pragma unroll
            for (int m = 0; m < MT; ++m)
#pragma unroll
                for (int kt = 0; kt < KT; ++kt) {
                    __syncthreads();
                    *reinterpret_cast<f32x4*>(&red[wave][lane * 4]) = dgacc[m][kt];
                    __syncthreads();
                    const int ln = tid >> 2, r = tid & 3;
                    const int u = u0 + 16 * m + 4 * (ln >> 4) + r, k = ks0 + kt * 16 + (ln & 15);
                    if (u <= U && kt < ktn)
                        a.dgp[(((size_t)chunk * U1 + u) * B + b) * J + k] = (red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid]);
                }
        }
    }
    __syncthreads();
    // df of the chunk's frames (zero rows past the utterance's length)
    for (int e = tid; e < (tc1 - tc0) * KS; e += RT_THREADS) {
        const int r = e / KS, kk = e % KS;
        if (ks0 + kk < J) a.df[((size_t)(tc0 + r) * B + b) * J + ks0 + kk] = dfl[r][kk];
    }
    // dW_out / db_out partial of this workgroup
#pragma unroll
    for (int kt = 0; kt < KT; ++kt)
#pragma unroll
        for (int q = 0; q < NT; ++q) {
            __syncthreads();
            *reinterpret_cast<f32x4*>(&red[wave][lane * 4]) = accW[kt][q];
            __syncthreads();
            const int ln = tid >> 2, r = tid & 3;
            const int k = ks0 + kt * 16 + 4 * (ln >> 4) + r, c = q * 16 + (ln & 15);
            if (kt < ktn && c < C) a.dwp[((size_t)item * J + k) * C + c] = (red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid]);
        }
    if (blockIdx.y == 0) {
        __syncthreads();
#pragma unroll
        for (int q = 0; q < NT; ++q) {
            float s = dbacc[q];
            s += __shfl_xor(s, 16, 64);
            s += __shfl_xor(s, 32, 64);
            if (lg == 0) red[wave][q * 16 + li] = s;
        }
        __syncthreads();
        if (tid < CP && tid < C) a.dbp[(size_t)item * C + tid] = (red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid]);
    }
}

// dg[u][b][:] = the chunk partials in chunk order; rows without a live node are zero
__global__ __launch_bounds__(RT_THREADS) void rnnt_reduce_dg_kernel(BwdArgs a) {
    const size_t e = (size_t)blockIdx.x * RT_THREADS + threadIdx.x;
    const size_t per = (size_t)(a.U + 1) * a.B * a.J;
    if (e >= per) return;
    const int b = (int)((e / a.J) % a.B), u = (int)(e / ((size_t)a.J * a.B));
    const int Tb = rt_clampi(a.lengths[b], 0, a.T), nb = rt_clampi(a.n[b], 0, a.U);
    float s = 0.0f;
    if (u <= nb)
        for (int c = 0; c < a.t_chunks && c * a.tc < Tb; ++c) s += a.dgp[(size_t)c * per + e];
    a.dg[e] = s;
}

// dW_out += the workgroup partials in item order, db_out likewise
__global__ __launch_bounds__(RT_THREADS) void rnnt_reduce_dw_kernel(BwdArgs a) {
    const size_t e = (size_t)blockIdx.x * RT_THREADS + threadIdx.x;
    const size_t jc = (size_t)a.J * a.C;
    if (e < jc) {
        float s = 0.0f;
        for (int i = 0; i < a.items; ++i) s += a.dwp[(size_t)i * jc + e];
        a.dw[e] += s;
    } else if (e < jc + a.C) {
        const int c = (int)(e - jc);
        float s = 0.0f;
        for (int i = 0; i < a.items; ++i) s += a.dbp[(size_t)i * a.C + c];
        a.db[c] += s;
    }
}

// ---------------------------------------------------------------------------------------------------------------- greedy decoding
// One iteration of time-synchronous greedy decoding, one workgroup per utterance (B rows of latency, nothing to tile): the
// prediction projection of the row's current state, the joint row at its frame, the argmax (ties to the smallest class), and the
// row's (parent, token, dest) entry for the amdspeech_lm_step_state call that follows.  Every sum runs in increasing k in one thread.
struct GreedyArgs {
    int T, B, U, J, C, L, H;
    const float *f, *pool_h, *w_pred, *b_pred, *w_out, *b_out;
    const int* lengths;
    int *t_idx, *m, *slot, *ids, *parent, *token, *dest;
};

__global__ __launch_bounds__(RT_THREADS) void rnnt_greedy_step_kernel(GreedyArgs a) {
#pragma clang fp contract(off)
    __shared__ float z[RT_J_MAX];
    __shared__ float lg[RT_C_MAX];
    const int tid = threadIdx.x, b = blockIdx.x;
    const int Tb = rt_clampi(a.lengths[b], 0, a.T);
    const int t = a.t_idx[b], m = a.m[b], sl = a.slot[b];
    if (t < 0 || t >= Tb || m < 0 || m >= a.U || sl < 2 * b || sl > 2 * b + 1) {      // finished (or not a state of this call): a no-op
        if (tid == 0) { a.parent[b] = -1; a.token[b] = 0; a.dest[b] = -1; }
        return;
    }
    const float* h = a.pool_h + ((size_t)sl * a.L + (a.L - 1)) * a.H;
    const float* fr = a.f + ((size_t)t * a.B + b) * a.J;
    for (int j = tid; j < a.J; j += RT_THREADS) {
        float s = 0.0f;
        for (int k = 0; k < a.H; ++k) s = fmaf(h[k], a.w_pred[(size_t)k * a.J + j], s);
        z[j] = tanhf(fr[j] + (s + a.b_pred[j]));
    }
    __syncthreads();
    for (int c = tid; c < a.C; c += RT_THREADS) {
        float s = 0.0f;
        for (int k = 0; k < a.J; ++k) s = fmaf(z[k], a.w_out[(size_t)k * a.C + c], s);
        lg[c] = s + a.b_out[c];
    }
    __syncthreads();
    if (tid == 0) {
        int best = 0;
        float bv = lg[0];
        for (int c = 1; c < a.C; ++c)
            if (lg[c] > bv) { bv = lg[c]; best = c; }
        if (best == a.C - 1) {
            a.t_idx[b] = t + 1;
            a.parent[b] = sl; a.token[b] = 0; a.dest[b] = -1;
        } else {
            a.ids[(size_t)b * a.U + m] = best;
            a.m[b] = m + 1;
            a.parent[b] = sl; a.token[b] = best; a.dest[b] = sl ^ 1;      // the row's two slots are 2 b and 2 b + 1
            a.slot[b] = sl ^ 1;
        }
    }
}

template <int MT, int NT>
static void launch_joint_fwd(hipStream_t s, const RnntPlan& p, const JointArgs& a) {
    hipLaunchKernelGGL((rnnt_joint_fwd_kernel<MT, NT>), dim3(p.fwd_grid), dim3(RT_THREADS), 0, s, a);
}
template <int NT, int KT>
static void launch_joint_bwd(hipStream_t s, const RnntPlan& p, const BwdArgs& a) {
    hipLaunchKernelGGL((rnnt_joint_bwd_kernel<NT, KT>), dim3(p.bwd_items, p.bwd_k_slices), dim3(RT_THREADS), 0, s, a);
}

}  // namespace amdspeech

using namespace amdspeech;

extern "C" int amdspeech_rnnt_plan(int T, int B, int U, int J, int C, amdspeech_rnnt_plan_info* out) {
    AS_CHECK_ARG(out != nullptr, "rnnt_plan: null output");
    return plan_rnnt(T, B, U, J, C, out);
}

extern "C" size_t amdspeech_rnnt_workspace_bytes(int T, int B, int U, int J, int C) {
    RnntPlan p;
    if (plan_rnnt(T, B, U, J, C, &p)) return 0;
    return ws_layout(T, B, U, J, C, p).total;
}

extern "C" int amdspeech_rnnt_targets(void* stream, const int* dense_labels, int B, int U, int C, int* targets, int* n, int* tok,
                                      int* tok_len) {
    RnntPlan p;
    if (int rc = plan_rnnt(1, B, U, 16, C, &p)) return rc;
    AS_CHECK_ARG(dense_labels && targets && n && tok && tok_len, "rnnt_targets: null pointer");
    hipLaunchKernelGGL(rnnt_targets_kernel, dim3(B), dim3(64), 0, static_cast<hipStream_t>(stream), dense_labels, U, C, targets, n, tok,
                       tok_len);
    AS_CHECK_LAUNCH();
    return AMDSPEECH_OK;
}

extern "C" int amdspeech_rnnt_joint_fwd(void* stream, const float* f, const float* g, const float* w_out, const float* b_out,
                                        const int* lengths, const int* n, int T, int B, int U, int J, int C, float* logits) {
    RnntPlan p;
    if (int rc = plan_rnnt(T, B, U, J, C, &p)) return rc;
    AS_CHECK_ARG(f && g && w_out && b_out && lengths && n && logits, "rnnt_joint_fwd: null pointer");
    JointArgs a;
    a.T = T; a.B = B; a.U = U; a.J = J; a.C = C;
    a.t_tiles = p.fwd_t_tiles; a.u_tiles = p.fwd_u_tiles;
    a.f = f; a.g = g; a.w = w_out; a.bias = b_out; a.lengths = lengths; a.n = n; a.logits = logits;
    hipStream_t s = static_cast<hipStream_t>(stream);
    switch (p.col_tiles) {
        case 2: launch_joint_fwd<4, 2>(s, p, a); break;
        case 5: launch_joint_fwd<4, 5>(s, p, a); break;
        case 8: launch_joint_fwd<2, 8>(s, p, a); break;
        default: launch_joint_fwd<1, 16>(s, p, a); break;
    }
    AS_CHECK_LAUNCH();
    return AMDSPEECH_OK;
}

extern "C" int amdspeech_rnnt_loss_fwd_bwd(void* stream, const float* logits, const int* targets, const int* n, const int* lengths,
                                           int T, int B, int U, int C, float* loss, float* dlogits, void* ws) {
    RnntPlan p;
    if (int rc = plan_rnnt(T, B, U, 16, C, &p)) return rc;
    AS_CHECK_ARG(logits && targets && n && lengths && loss && dlogits && ws, "rnnt_loss: null pointer");
    AS_CHECK_ARG((reinterpret_cast<uintptr_t>(ws) & 255) == 0, "rnnt_loss: the workspace must be 256-byte aligned");
    const RnntWs w = ws_layout(T, B, U, 16, C, p);      // (the regions the loss uses lie in front of those that depend on J)
    char* base = static_cast<char*>(ws);
    LossArgs a;
    a.T = T; a.B = B; a.U = U; a.C = C;
    a.logits = logits; a.targets = targets; a.n = n; a.lengths = lengths;
    a.lpb = reinterpret_cast<float*>(base + w.lpb); a.lpy = reinterpret_cast<float*>(base + w.lpy);
    a.alpha = reinterpret_cast<double*>(base + w.alpha); a.beta = reinterpret_cast<double*>(base + w.beta);
    a.lnp = reinterpret_cast<double*>(base + w.lnp);
    a.loss = loss; a.dlogits = dlogits;
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(rnnt_rows_kernel, dim3(p.rows_grid), dim3(RT_THREADS), 0, s, a);
    AS_CHECK_LAUNCH();
    switch (p.rec_kernel) {
        case AMDSPEECH_RNNT_REC_WAVE: hipLaunchKernelGGL((rnnt_lattice_kernel<64, 1>), dim3(p.rec_grid), dim3(64), 0, s, a); break;
        case AMDSPEECH_RNNT_REC_BLOCK1: hipLaunchKernelGGL((rnnt_lattice_kernel<256, 1>), dim3(p.rec_grid), dim3(256), 0, s, a); break;
        case AMDSPEECH_RNNT_REC_BLOCK4: hipLaunchKernelGGL((rnnt_lattice_kernel<256, 4>), dim3(p.rec_grid), dim3(256), 0, s, a); break;
        default: hipLaunchKernelGGL((rnnt_lattice_kernel<256, 10>), dim3(p.rec_grid), dim3(256), 0, s, a); break;
    }
    AS_CHECK_LAUNCH();
    hipLaunchKernelGGL(rnnt_grad_kernel, dim3(p.rows_grid), dim3(RT_THREADS), 0, s, a);
    AS_CHECK_LAUNCH();
    return AMDSPEECH_OK;
}

extern "C" int amdspeech_rnnt_joint_bwd(void* stream, const float* dlogits, const float* f, const float* g, const float* w_out,
                                        const int* lengths, const int* n, int T, int B, int U, int J, int C, float* df, float* dg,
                                        float* dw_out, float* db_out, void* ws) {
    RnntPlan p;
    if (int rc = plan_rnnt(T, B, U, J, C, &p)) return rc;
    AS_CHECK_ARG(dlogits && f && g && w_out && lengths && n && df && dg && dw_out && db_out && ws, "rnnt_joint_bwd: null pointer");
    AS_CHECK_ARG((reinterpret_cast<uintptr_t>(ws) & 255) == 0, "rnnt_joint_bwd: the workspace must be 256-byte aligned");
    AS_CHECK_ARG(p.bwd_k_slices <= 65535, "rnnt_joint_bwd: grid too large");
    const RnntWs w = ws_layout(T, B, U, J, C, p);
    char* base = static_cast<char*>(ws);
    BwdArgs a;
    a.T = T; a.B = B; a.U = U; a.J = J; a.C = C;
    a.tc = p.bwd_t_chunk; a.t_chunks = p.bwd_t_chunks; a.items = p.bwd_items;
    a.dl = dlogits; a.f = f; a.g = g; a.w = w_out; a.lengths = lengths; a.n = n;
    a.df = df; a.dg = dg; a.dw = dw_out; a.db = db_out;
    a.dgp = reinterpret_cast<float*>(base + w.dgp); a.dwp = reinterpret_cast<float*>(base + w.dwp);
    a.dbp = reinterpret_cast<float*>(base + w.dbp);
    hipStream_t s = static_cast<hipStream_t>(stream);
    switch (p.col_tiles) {
        case 2: launch_joint_bwd<2, 4>(s, p, a); break;
        case 5: launch_joint_bwd<5, 4>(s, p, a); break;
        case 8: launch_joint_bwd<8, 2>(s, p, a); break;
        default: launch_joint_bwd<16, 1>(s, p, a); break;
    }
    AS_CHECK_LAUNCH();
    hipLaunchKernelGGL(rnnt_reduce_dg_kernel, dim3(p.reduce_dg_grid), dim3(RT_THREADS), 0, s, a);
    AS_CHECK_LAUNCH();
    hipLaunchKernelGGL(rnnt_reduce_dw_kernel, dim3(p.reduce_dw_grid), dim3(RT_THREADS), 0, s, a);
    AS_CHECK_LAUNCH();
    return AMDSPEECH_OK;
}

extern "C" int amdspeech_rnnt_greedy_step(void* stream, const float* f, const int* lengths, int T, int B, int U, int J, int C,
                                          const float* pool_h, int L, int H, const float* w_pred, const float* b_pred,
                                          const float* w_out, const float* b_out, int* t_idx, int* m, int* slot, int* ids, int* parent,
                                          int* token, int* dest) {
    RnntPlan p;
    if (int rc = plan_rnnt(T, B, U, J, C, &p)) return rc;
    AS_CHECK_ARG(L >= 1 && L <= 8, "rnnt_greedy_step: L = %d outside 1 .. 8", L);
    AS_CHECK_ARG(H >= 1, "rnnt_greedy_step: H = %d must be positive", H);
    if ((long long)2 * B * L * H >= (1LL << 31)) {
        set_error("rnnt_greedy_step: 2 * B * L * H = %lld must be below 2^31", (long long)2 * B * L * H);
        return AMDSPEECH_EUNSUPPORTED;
    }
    AS_CHECK_ARG(f && lengths && pool_h && w_pred && b_pred && w_out && b_out && t_idx && m && slot && ids && parent && token && dest,
                 "rnnt_greedy_step: null pointer");
    GreedyArgs a;
    a.T = T; a.B = B; a.U = U; a.J = J; a.C = C; a.L = L; a.H = H;
    a.f = f; a.pool_h = pool_h; a.w_pred = w_pred; a.b_pred = b_pred; a.w_out = w_out; a.b_out = b_out; a.lengths = lengths;
    a.t_idx = t_idx; a.m = m; a.slot = slot; a.ids = ids; a.parent = parent; a.token = token; a.dest = dest;
    hipLaunchKernelGGL(rnnt_greedy_step_kernel, dim3(B), dim3(RT_THREADS), 0, static_cast<hipStream_t>(stream), a);
    AS_CHECK_LAUNCH();
    return AMDSPEECH_OK;
}
