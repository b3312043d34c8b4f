// One language-model step for N hypotheses, each from its own parent state in a slot pool (amdspeech.h: amdspeech_lm_step;
// DESIGN.md 4.7): what the fused beam search (beam.cpp) calls once per frame.  No reference counterpart: the reference never
// decodes with its language model.
//
// Regime.  N is a few hundred rows (the hypotheses that entered a beam this frame, over the mini-batch), the layer's weights are
// [2H][4H] f32 (2 MB at H 256, 8 MB at H 512): at N <= 64 the call is a stream of the weights out of L2 / Infinity Cache, above
// that an f32 product of N x 2H x 4H.  The whole-sequence LSTM kernels (one 512-thread workgroup per CU, persistent) are built for
// T steps of one batch and cannot gather a ragged set of parents; a single time step does not amortise them either.
//
// Structure: L + 1 plain launches, nothing waits across workgroups.
//   layer l    grid (row tiles, H / 16): a workgroup owns 16 MT rows (MT = 1 or 2) x 16 hidden units x the 4 gates.  The k range 2H is cut
//              into blocks of 16 that are dealt to the four waves (a fixed function of H); each wave runs
//              v_mfma_f32_16x16x4_f32 with the ROWS on the A port -- A fragments are gathered through parent / dest / token
//              while they are loaded (16 bytes per lane; x_0 = input_w[token] + input_b is formed in the load), B fragments
//              come straight from the kernel matrix -- and leaves its partial tile in LDS.  The epilogue adds the four partials in
//              a fixed order, then the bias, and does the cell update: the pre-activations never leave the chip.
//   output     grid (row tiles of 16): h'_top . output_w on the same instruction, k dealt to the four waves in the same way, eight
//              16-column tiles per pass (two passes above V 128), the partial tiles and then the logits through LDS, then
//              log-softmax with one wave per row (shuffles in a fixed order).
// A weight element is read once per ROW TILE, never once per row.
//
// Bit-for-bit row independence: the MFMA is a k-ordered fmaf chain per (row, column); the order of k -- block by block, inside a
// block the four lane groups interleaved -- and the split over the waves depend on H alone, and MT only changes how many row
// sub-tiles share the B fragments.  No atomics, no reduction whose order depends on N.
#include "common.h"

#include <math.h>

namespace amdspeech {

constexpr int LS_THREADS = 256;
constexpr int LS_WAVES = LS_THREADS / 64;
constexpr int LS_H_MAX = 4096;
constexpr int LS_V_MAX = 256;
constexpr int LS_L_MAX = 8;
constexpr int LS_N_MAX = (1 << 24) - 1;
constexpr int LS_OUT_NT = 8;                   // output layer: column tiles of 16 per pass
constexpr int LS_OUT_LD = LS_V_MAX + 1;        // logits tile in LDS: [16][V_MAX + 1] (odd stride: the column reads of a row do not collide)

typedef amdspeech_lm_step_plan_info StepPlan;

static int plan_lm_step(int N, int L, int H, int V, StepPlan* p) {
    AS_CHECK_ARG(N >= 1, "lm_step: N = %d must be positive", N);
    AS_CHECK_ARG(L >= 1 && L <= LS_L_MAX, "lm_step: L = %d outside 1 .. %d", L, LS_L_MAX);
    AS_CHECK_ARG(H >= 16 && H % 16 == 0, "lm_step: H = %d must be a positive multiple of 16", H);
    AS_CHECK_ARG(V >= 2, "lm_step: V = %d must be at least 2", V);
    if (H > LS_H_MAX) { set_error("lm_step: H = %d above the kernels' limit of %d", H, LS_H_MAX); return AMDSPEECH_EUNSUPPORTED; }
    if (V > LS_V_MAX) { set_error("lm_step: V = %d above the kernels' limit of %d", V, LS_V_MAX); return AMDSPEECH_EUNSUPPORTED; }
    if (N > LS_N_MAX) { set_error("lm_step: N = %d above the kernels' limit of %d", N, LS_N_MAX); return AMDSPEECH_EUNSUPPORTED; }
    // Row sub-tiles per workgroup.  One below 65 rows: the call is the weight stream there, and more workgroups pull it faster;
    // two above, where the product dominates and a B fragment feeds two row sub-tiles.  (Four were measured at N = 3200: 171 us
    // against 155 us per call at 2 x 256, 501 against 468 at 2 x 512 -- 64 KiB of LDS leave two workgroups per CU -- and dropped.)
    const int mt = N <= 64 ? 1 : 2;
    p->kernel = AMDSPEECH_LM_STEP_KERNEL_MFMA16;
    p->row_tile = 16 * mt;
    p->threads = LS_THREADS;
    p->launches = L + 1;
    p->n_min = mt == 1 ? 1 : 65;
    p->n_max = mt == 1 ? 64 : LS_N_MAX;
    p->col_tiles = H / 16;
    p->row_tiles = ceil_div(N, p->row_tile);
    p->lds_bytes = LS_WAVES * mt * 4 * 256 * 4;
    p->out_row_tile = 16;
    p->out_row_tiles = ceil_div(N, 16);
    p->v_max = LS_V_MAX;
    return AMDSPEECH_OK;
}

struct StepArgs {
    int N, n_slots, L, H, V, layer;
    const int *parent, *token, *dest;
    float *pool_h, *pool_c;
    const float *input_w, *input_b, *kernel, *bias, *output_w, *output_b;
    float* logq;
};

__device__ __forceinline__ float ls_sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }

// ------------------------------------------------------------------------------------------------------------ one layer
template <int MT>
__global__ __launch_bounds__(LS_THREADS) void lm_step_layer_kernel(StepArgs a) {
#pragma clang fp contract(off)      // every rounding as written: the instantiations must give a row the same bits
    __shared__ __attribute__((aligned(16))) float red[LS_WAVES][MT * 4][256];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int H = a.H, L = a.L, l = a.layer;
    const int row0 = blockIdx.x * (16 * MT), j0 = blockIdx.y * 16;
    const int li = lane & 15, lg = lane >> 4;
    const f32x4 zero4 = {0.0f, 0.0f, 0.0f, 0.0f};

    // the A rows of this lane: where x and h of row (row0 + 16 m + li) come from.  A row without a source (past N, parent -1, an
    // index outside its range) keeps a valid address and a false flag: the loads stay unconditional -- a predicated load costs a
    // branch and a wait of its own -- and the data is zeroed by a select.
    const float* xsrc[MT];
    const float* hsrc[MT];
    bool xok[MT], hok[MT];
#pragma unroll
    for (int m = 0; m < MT; ++m) {
        const int r = row0 + 16 * m + li;
        xsrc[m] = l == 0 ? a.input_w : a.pool_h;
        hsrc[m] = a.pool_h;
        xok[m] = hok[m] = false;
        if (r < a.N) {
            const int par = a.parent[r], dst = a.dest[r];
            if (par >= 0 && par < a.n_slots) { hsrc[m] = a.pool_h + ((size_t)par * L + l) * H; hok[m] = true; }
            if (l == 0) {
                const int tk = a.token[r];
                if (tk >= 0 && tk < a.V) { xsrc[m] = a.input_w + (size_t)tk * H; xok[m] = true; }
            } else if (dst >= 0 && dst < a.n_slots) {
                xsrc[m] = a.pool_h + ((size_t)dst * L + (l - 1)) * H;
                xok[m] = true;
            }
        }
    }
    f32x4 acc[MT][4];
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int g = 0; g < 4; ++g) acc[m][g] = zero4;

    const int nkb = H / 8;                                   // blocks of 16 k in 2H
    const int kb0 = wave * nkb / LS_WAVES, kb1 = (wave + 1) * nkb / LS_WAVES;
    const float* wcol = a.kernel + j0 + li;                  // column j0 + li of gate 0
    // UN blocks per burst, two register sets: the loads of the next burst are in flight under the MFMAs of this one (the operands
    // come from L2 / Infinity Cache, a microsecond away: memory-level parallelism is what bounds a wave here).  A block past the
    // wave's range loads a clamped address and is not multiplied: a row's fmaf chain is the same at every UN and MT.
    constexpr int UN = MT == 1 ? 4 : 2;
    static_assert(MT == 1 || MT == 2, "row sub-tiles per workgroup");
    auto load_burst = [&](int kbs, f32x4 (&av)[UN][MT], float (&bv)[UN][4][4]) {
#pragma unroll
        for (int u = 0; u < UN; ++u) {
            const int kb = kbs + u < kb1 ? kbs + u : kb1 - 1;
            const int k0 = kb * 16 + 4 * lg;                 // this lane's four k of the block
            const bool isx = k0 < H;
#pragma unroll
            for (int m = 0; m < MT; ++m) {
                const float* src = isx ? xsrc[m] : hsrc[m];
                const bool ok = isx ? xok[m] : hok[m];
                const int kk = isx ? k0 : k0 - H;
                f32x4 v = *reinterpret_cast<const f32x4*>(src + kk);
                v = ok ? v : zero4;
                if (l == 0) {                                // x_0 = input_w[token] + input_b: ONE rounding, as embed_fwd
                    const f32x4 b = *reinterpret_cast<const f32x4*>(a.input_b + (isx ? kk : 0));
                    const f32x4 xb = row0 + 16 * m + li < a.N ? (ok ? v + b : b) : zero4;
                    v = isx ? xb : v;
                }
                av[u][m] = v;
            }
#pragma unroll
            for (int s = 0; s < 4; ++s)
#pragma unroll
                for (int g = 0; g < 4; ++g) bv[u][g][s] = wcol[(size_t)(k0 + s) * 4 * H + g * H];
        }
    };
    auto mma_burst = [&](int kbs, const f32x4 (&av)[UN][MT], const float (&bv)[UN][4][4]) {
#pragma unroll
        for (int u = 0; u < UN; ++u) {
            if (kbs + u >= kb1) break;                       // (uniform over the wave)
#pragma unroll
            for (int s = 0; s < 4; ++s)
#pragma unroll
                for (int m = 0; m < MT; ++m)
#pragma unroll
                    for (int g = 0; g < 4; ++g)
                        acc[m][g] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[u][m][s], bv[u][g][s], acc[m][g], 0, 0, 0);
        }
    };
    if (kb1 > kb0) {                                         // (a wave's range is empty at H = 16)
        f32x4 a0[UN][MT], a1[UN][MT];
        float b0[UN][4][4], b1[UN][4][4];
        load_burst(kb0, a0, b0);
        for (int kbs = kb0; kbs < kb1; kbs += 2 * UN) {
            load_burst(kbs + UN, a1, b1);
            __builtin_amdgcn_sched_barrier(0);
            mma_burst(kbs, a0, b0);
            load_burst(kbs + 2 * UN, a0, b0);
            __builtin_amdgcn_sched_barrier(0);
            mma_burst(kbs + UN, a1, b1);
        }
    }
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int g = 0; g < 4; ++g) *reinterpret_cast<f32x4*>(&red[wave][m * 4 + g][lane * 4]) = acc[m][g];
    __syncthreads();

    // epilogue: thread (i, j) of the 16 x 16 tile, MT rows each; D[i][j] sits at lane (i / 4) * 16 + j, register i % 4
    const int i = tid >> 4, j = tid & 15;
    const int e = ((i >> 2) * 16 + j) * 4 + (i & 3);
    const int unit = j0 + j;
    float bias[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) bias[g] = a.bias[g * H + unit];
#pragma unroll
    for (int m = 0; m < MT; ++m) {
        const int r = row0 + 16 * m + i;
        if (r >= a.N) continue;
        const int par = a.parent[r], dst = a.dest[r];
        if (dst < 0 || dst >= a.n_slots) continue;
        float pre[4];
#pragma unroll
        for (int g = 0; g < 4; ++g)
            pre[g] = ((red[0][m * 4 + g][e] + red[1][m * 4 + g][e]) + (red[2][m * 4 + g][e] + red[3][m * 4 + g][e])) + bias[g];
        float cp = 0.0f;
        if (par >= 0 && par < a.n_slots) cp = a.pool_c[((size_t)par * L + l) * H + unit];
        const float gi = ls_sigmoid(pre[0]);
        const float gj = tanhf(pre[1]);
        const float gf = ls_sigmoid(pre[2] + 1.0f);          // forget bias 1.0, added at run time
        const float go = ls_sigmoid(pre[3]);
        const float cn = fmaf(cp, gf, gi * gj);              // spelled out: with contraction left to the compiler the
        const float hn = tanhf(cn) * go;                     // instantiations may round c' differently (see the pragma above)
        const size_t o = ((size_t)dst * L + l) * H + unit;
        a.pool_c[o] = cn;
        a.pool_h[o] = hn;
    }
}

// --------------------------------------------------------------------------------------- output layer and log-softmax
__global__ __launch_bounds__(LS_THREADS) void lm_step_out_kernel(StepArgs a) {
#pragma clang fp contract(off)
    __shared__ float lgt[16][LS_OUT_LD];
    __shared__ __attribute__((aligned(16))) float red[LS_WAVES][LS_OUT_NT][256];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int H = a.H, L = a.L, V = a.V;
    const int row0 = blockIdx.x * 16;
    const int li = lane & 15, lg = lane >> 4;
    const f32x4 zero4 = {0.0f, 0.0f, 0.0f, 0.0f};
    const int ntile = (V + 15) / 16;

    const float* hsrc = a.pool_h;                                  // (unconditional loads, as in the layer kernel)
    bool hok = false;
    {
        const int r = row0 + li;
        if (r < a.N) {
            const int dst = a.dest[r];
            if (dst >= 0 && dst < a.n_slots) { hsrc = a.pool_h + ((size_t)dst * L + (L - 1)) * H; hok = true; }
        }
    }
    // k is dealt to the four waves in blocks of 16, as in the layer kernel (a fixed function of H); each wave covers up to
    // LS_OUT_NT column tiles at a time (V above 128: two passes), all loads of a burst of UN blocks in flight before the MFMAs
    const int nkb = H / 16;
    const int kb0 = wave * nkb / LS_WAVES, kb1 = (wave + 1) * nkb / LS_WAVES;
    constexpr int UN = 2;
    for (int t0 = 0; t0 < ntile; t0 += LS_OUT_NT) {
        f32x4 acc[LS_OUT_NT];
#pragma unroll
        for (int q = 0; q < LS_OUT_NT; ++q) acc[q] = zero4;
        for (int kbs = kb0; kbs < kb1; kbs += UN) {
            f32x4 av[UN];
            float bv[UN][LS_OUT_NT][4];
#pragma unroll
            for (int u = 0; u < UN; ++u) {
                const int kb = kbs + u < kb1 ? kbs + u : kb1 - 1;
                const int k0 = kb * 16 + 4 * lg;
                const f32x4 v = *reinterpret_cast<const f32x4*>(hsrc + k0);
                av[u] = hok ? v : zero4;
#pragma unroll
                for (int q = 0; q < LS_OUT_NT; ++q) {
                    const int col = (t0 + q) * 16 + li, colc = col < V ? col : V - 1;      // clamped address, the data zeroed
#pragma unroll
                    for (int s = 0; s < 4; ++s) {
                        const float w = a.output_w[(size_t)(k0 + s) * V + colc];
                        bv[u][q][s] = col < V ? w : 0.0f;
                    }
                }
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int u = 0; u < UN; ++u) {
                if (kbs + u >= kb1) break;                         // (uniform over the wave)
#pragma unroll
                for (int s = 0; s < 4; ++s)
#pragma unroll
                    for (int q = 0; q < LS_OUT_NT; ++q)            // (a tile past V multiplies zeros: no branch between the MFMAs)
                        acc[q] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[u][s], bv[u][q][s], acc[q], 0, 0, 0);
            }
        }
#pragma unroll
        for (int q = 0; q < LS_OUT_NT; ++q) *reinterpret_cast<f32x4*>(&red[wave][q][lane * 4]) = acc[q];
        __syncthreads();
        {   // thread (i, j) of every 16 x 16 tile: the four partials in a fixed order, then the bias
            const int i = tid >> 4, j = tid & 15;
            const int e = ((i >> 2) * 16 + j) * 4 + (i & 3);
#pragma unroll
            for (int q = 0; q < LS_OUT_NT; ++q) {
                const int col = (t0 + q) * 16 + j;
                if (col < V) lgt[i][col] = ((red[0][q][e] + red[1][q][e]) + (red[2][q][e] + red[3][q][e])) + a.output_b[col];
            }
        }
        __syncthreads();                                           // (red is written again by the next pass; lgt is read below)
    }
    // one wave per row, four rows each: lane holds columns lane + 64 q
    for (int rr = 0; rr < 4; ++rr) {
        const int i = wave * 4 + rr, r = row0 + i;
        if (r >= a.N) break;                                   // (uniform over the wave)
        const int dst = a.dest[r];
        if (dst < 0 || dst >= a.n_slots) continue;
        float x[4], m = -INFINITY;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int c = lane + 64 * q;
            x[q] = c < V ? lgt[i][c] : -INFINITY;
            m = fmaxf(m, x[q]);
        }
        for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
        float s = 0.0f;
#pragma unroll
        for (int q = 0; q < 4; ++q) s += lane + 64 * q < V ? expf(x[q] - m) : 0.0f;
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
        const float lse = m + logf(s);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int c = lane + 64 * q;
            if (c < V) a.logq[(size_t)r * V + c] = x[q] - lse;
        }
    }
}

static bool ls_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace amdspeech

using namespace amdspeech;

extern "C" int amdspeech_lm_step_plan(int N, int L, int H, int V, amdspeech_lm_step_plan_info* out) {
    AS_CHECK_ARG(out != nullptr, "lm_step_plan: null output");
    return plan_lm_step(N, L, H, V, out);
}

extern "C" size_t amdspeech_lm_step_pool_bytes(int n_slots, int L, int H) {
    StepPlan p;
    if (plan_lm_step(1, L, H, 2, &p)) return 0;
    if (n_slots < 1 || (long)n_slots * L * H >= (1L << 31)) {
        set_error("lm_step_pool_bytes: n_slots = %d must be positive with n_slots * L * H below 2^31", n_slots);
        return 0;
    }
    return (size_t)n_slots * L * H * sizeof(float);
}

// The L layer launches, and the output launch when `output` is set (amdspeech_lm_step; amdspeech_lm_step_state stops at the state)
static int lm_step_launch(void* stream, int N, const int* parent, const int* token, const int* dest, float* pool_h, float* pool_c,
                          int n_slots, int L, int H, int V, const float* input_w, const float* input_b, const float* kernel_0,
                          long kernel_stride, const float* bias_0, long bias_stride, bool output, const float* output_w,
                          const float* output_b, float* logq) {
    StepPlan p;
    if (int rc = plan_lm_step(N, L, H, V, &p)) return rc;
    AS_CHECK_ARG(parent && token && dest && pool_h && pool_c && input_w && input_b && kernel_0 && bias_0 &&
                     (!output || (output_w && output_b && logq)),
                 "lm_step: null pointer");
    AS_CHECK_ARG(n_slots >= 1 && (long)n_slots * L * H < (1L << 31), "lm_step: n_slots = %d must be positive with n_slots * L * H below 2^31",
                 n_slots);
    AS_CHECK_ARG(pool_h != pool_c, "lm_step: pool_h and pool_c are the same buffer");
    AS_CHECK_ARG(ls_aligned16(pool_h) && ls_aligned16(pool_c) && ls_aligned16(input_w) && ls_aligned16(input_b) && ls_aligned16(kernel_0) &&
                     ls_aligned16(bias_0),
                 "lm_step: the pool, input_w, input_b, kernel_0 and bias_0 must be 16-byte aligned");
    AS_CHECK_ARG(L == 1 || (kernel_stride >= (long)2 * H * 4 * H && bias_stride >= (long)4 * H && kernel_stride % 4 == 0 && bias_stride % 4 == 0),
                 "lm_step: kernel_stride = %ld / bias_stride = %ld must cover a layer and be multiples of 4 floats", kernel_stride, bias_stride);
    AS_CHECK_ARG(p.row_tiles <= 0x7fffffff / 2 && p.col_tiles <= 65535, "lm_step: grid too large");
    hipStream_t s = static_cast<hipStream_t>(stream);
    StepArgs a;
    a.N = N; a.n_slots = n_slots; a.L = L; a.H = H; a.V = V;
    a.parent = parent; a.token = token; a.dest = dest;
    a.pool_h = pool_h; a.pool_c = pool_c;
    a.input_w = input_w; a.input_b = input_b; a.output_w = output_w; a.output_b = output_b;
    a.logq = logq;
    a.layer = 0; a.kernel = kernel_0; a.bias = bias_0;
    for (int l = 0; l < L; ++l) {
        a.layer = l;
        a.kernel = kernel_0 + (size_t)l * kernel_stride;
        a.bias = bias_0 + (size_t)l * bias_stride;
        const dim3 grid(p.row_tiles, p.col_tiles), block(p.threads);
        if (p.row_tile == 16) hipLaunchKernelGGL(lm_step_layer_kernel<1>, grid, block, 0, s, a);
        else hipLaunchKernelGGL(lm_step_layer_kernel<2>, grid, block, 0, s, a);
        AS_CHECK_LAUNCH();
    }
    if (!output) return AMDSPEECH_OK;
    hipLaunchKernelGGL(lm_step_out_kernel, dim3(p.out_row_tiles), dim3(p.threads), 0, s, a);
    AS_CHECK_LAUNCH();
    return AMDSPEECH_OK;
}

extern "C" int amdspeech_lm_step(void* stream, int N, const int* parent, const int* token, const int* dest, float* pool_h, float* pool_c,
                                 int n_slots, int L, int H, int V, const float* input_w, const float* input_b, const float* kernel_0,
                                 long kernel_stride, const float* bias_0, long bias_stride, const float* output_w,
                                 const float* output_b, float* logq) {
    return lm_step_launch(stream, N, parent, token, dest, pool_h, pool_c, n_slots, L, H, V, input_w, input_b, kernel_0, kernel_stride, bias_0,
                          bias_stride, true, output_w, output_b, logq);
}

extern "C" int amdspeech_lm_step_state(void* stream, int N, const int* parent, const int* token, const int* dest, float* pool_h,
                                       float* pool_c, int n_slots, int L, int H, int V, const float* input_w, const float* input_b,
                                       const float* kernel_0, long kernel_stride, const float* bias_0, long bias_stride) {
    return lm_step_launch(stream, N, parent, token, dest, pool_h, pool_c, n_slots, L, H, V, input_w, input_b, kernel_0, kernel_stride, bias_0,
                          bias_stride, false, nullptr, nullptr, nullptr);
}
