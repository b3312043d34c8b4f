// Layer-wise bidirectional stacks in split precision (bf16x3, desc.precision = 1): the forward and backward recurrence kernels of
// one layer, both directions.  Included from lstm.hip after lstm_layer.h (namespace amdspeech); bf16_split / BF3_MMA come from
// lstm_step_bf3.h, the hand-off (layer_wait / layer_publish) and the dropout mask from lstm_layer.h.
//
// Same contract as lstm_layer_fwd / lstm_layer_bwd: step order with `rev`, frames past len_b copy the state through and emit 0,
// the output mask from the same (seed, stream, index), h0 / c0 for the forward cells only, [s0, s1) for the per-frame fallback,
// bounded waits that set the error word.  The gates, c, the f32 h / gate / dG histories stay f32 where the f32 kernels put them.
// What changes is the recurrent product, C[rows][N] = A[rows][K] . S[K][N] on v_mfma_f32_16x16x32_bf16 as hi.hi + hi.lo + lo.hi:
//   forward:  A = h_{s-1} [B][H],   S = the workgroup's W_hh columns [H][4 x 8 units]      (N = 32: two 16-column tiles)
//   backward: A = dG_{s+1} [B][4H], S = W_hh^T rows of its units [4H][16 units]            (N = 16: one tile)
// Each operand is split ONCE:
//   - S: every wave splits its K share of the slice when the launch starts and keeps it in registers (B-fragment order) for the
//     whole sequence -- KPW K-blocks of 32 per wave, 8 VGPRs per K-block and 16-column tile;
//   - A: the workgroup that produces a value (the cell that computed it) splits it and publishes it, hi / lo, in A-fragment
//     order (packed_off3: per 16-row tile and 32-wide K-block 1 KiB hi + 1 KiB lo) into a two-slot ring per direction.  Two
//     slots suffice under the counter protocol: a workgroup writes slot (s+1)&1 only after every workgroup of its direction has
//     published step s, which each did after reading slot (s-1)&1 = (s+1)&1.  Consumers read it with no conversion.
// Workgroup shape: K split over the waves (NW = K-blocks / KPW), partial tiles reduced through LDS, then one
// thread per (row, unit) cell.  Forward: 8 units x 64 rows (MB = 4 row tiles), backward: 16 units x 32 rows (MB = 2) -- at
// 5x1024 / B 64 both are 128 workgroups per direction, one per CU, and a backward workgroup reads half of the 1 MiB dG panel.
// PREC = 2 (plain bf16: hi.hi only, no lo half) is the template argument a plain-bf16 layer mode would instantiate.

constexpr int LBF3_FWD_U = 8, LBF3_FWD_NT = 2, LBF3_FWD_MB = 4, LBF3_FWD_MAXW = 8;
constexpr int LBF3_BWD_U = 16, LBF3_BWD_NT = 1, LBF3_BWD_MB = 2, LBF3_BWD_MAXW = 8;

struct LayerBf3Args {
    LayerArgs a;
    uint4* ring[2];       // per direction: two slots of the loop-carried operand (h forward, dG backward), split, A-fragment order
    int ngrp;             // row groups (MB row tiles each) per block of units
};

__device__ __forceinline__ void lbf3_split8(const float (&v)[8], uint4& hi, uint4& lo) {
    unsigned short h[8], l[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) bf16_split(v[e], h[e], l[e]);
    hi = make_uint4(h[0] | (unsigned)h[1] << 16, h[2] | (unsigned)h[3] << 16, h[4] | (unsigned)h[5] << 16, h[6] | (unsigned)h[7] << 16);
    lo = make_uint4(l[0] | (unsigned)l[1] << 16, l[2] | (unsigned)l[3] << 16, l[4] | (unsigned)l[5] << 16, l[6] | (unsigned)l[7] << 16);
}

template <int PREC>
__device__ __forceinline__ void lbf3_mma(f32x4& acc, const uint4& ah, const uint4& al, const uint4& bh, const uint4& bl) {
    if constexpr (PREC == 2)
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, ah), __builtin_bit_cast(bf16x8, bh), acc, 0, 0, 0);
    else
        BF3_MMA(acc, ah, al, bh, bl);
}

// acc[m][nt] = rows of tile mt0 + m of the panel (K-blocks [kb0, kb0 + KPW)) . this wave's slice fragments; tiles >= nmt stay 0.
// The A fragments stream in bursts of CH K-blocks, double-buffered: the loads of burst b + 1 are in flight while the MFMAs of
// burst b run.  The scheduling barriers keep hipcc from hoisting every burst's loads to the top (at KPW = 16 that spills).
template <int KPW, int MB, int NT, int PREC>
__device__ __forceinline__ void lbf3_product(const uint4* __restrict__ panel, int nkb, int mt0, int nmt, int kb0, int lane,
                                             const uint4 (&wh)[KPW][NT], const uint4 (&wl)[KPW][NT], f32x4 (&acc)[MB][NT]) {
    // K-blocks per burst (KPW 16: 128 VGPRs of S already), bursts per row tile
    constexpr int CH = KPW < 4 ? KPW : (KPW < 16 ? 4 : 2), NB = KPW / CH;
    const int mv = min(MB, nmt - mt0);                         // row tiles inside the batch (wave-uniform)
#pragma unroll
    for (int m = 0; m < MB; ++m)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) acc[m][nt] = (f32x4){0.f, 0.f, 0.f, 0.f};
    uint4 ah[2][CH], al[2][CH];
    auto load = [&](int b, int buf) {
        const int m = b / NB, k0 = (b % NB) * CH;
        if (m >= mv) return;
        const uint4* p = panel + ((size_t)(mt0 + m) * nkb + kb0 + k0) * 128 + lane;
#pragma unroll
        for (int q = 0; q < CH; ++q) {
            ah[buf][q] = p[q * 128];
            if constexpr (PREC != 2) al[buf][q] = p[q * 128 + 64];
            else al[buf][q] = ah[buf][q];
        }
    };
    load(0, 0);
#pragma unroll
    for (int b = 0; b < MB * NB; ++b) {
        if (b + 1 < MB * NB) load(b + 1, (b + 1) & 1);
        __builtin_amdgcn_sched_barrier(0);
        const int m = b / NB, k0 = (b % NB) * CH;
        if (m < mv) {
#pragma unroll
            for (int q = 0; q < CH; ++q)
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) lbf3_mma<PREC>(acc[m][nt], ah[b & 1][q], al[b & 1][q], wh[k0 + q][nt], wl[k0 + q][nt]);
        }
        __builtin_amdgcn_sched_barrier(0);
    }
}

// every wave's partial tiles -> LDS red[wave][m * NT + nt][256] (C/D order: lane * 4 + i = C[4 (lane >> 4) + i][lane & 15])
template <int MB, int NT>
__device__ __forceinline__ void lbf3_stage(float* red, int wv, int lane, const f32x4 (&acc)[MB][NT]) {
#pragma unroll
    for (int m = 0; m < MB; ++m)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
            *reinterpret_cast<f32x4*>(red + ((size_t)(wv * MB + m) * NT + nt) * 256 + lane * 4) = acc[m][nt];
}
// element (row i of tile m, column c) of the product, summed over the nw waves' K shares
template <int MB, int NT>
__device__ __forceinline__ float lbf3_sum(const float* red, int nw, int m, int i, int c) {
    const int e = (m * NT + (c >> 4)) * 256 + ((i >> 2) * 16 + (c & 15)) * 4 + (i & 3);
    float v = 0.f;
    for (int w = 0; w < nw; ++w) v += red[(size_t)w * MB * NT * 256 + e];
    return v;
}

// Forward recurrence of one layer, steps [s0, s1), both directions: grid = ndir x (H / 8) x ngrp workgroups of NW = H / 32 / KPW
// waves.  LDS: NW x MB x NT KiB (the partial tiles).
template <int KPW, int PREC>
__global__ __launch_bounds__(LBF3_FWD_MAXW * 64) void lstm_layer_fwd_bf3(LayerBf3Args x) {
    extern __shared__ float4 lbf3_lds4[];
    float* red = reinterpret_cast<float*>(lbf3_lds4);
    __shared__ int abort_flag;
    constexpr int U = LBF3_FWD_U, NT = LBF3_FWD_NT, MB = LBF3_FWD_MB;
    const LayerArgs& a = x.a;
    const int H = a.H, B = a.B, nub = H / U, nwg = nub * x.ngrp;
    const int dn = blockIdx.x / nwg, r = blockIdx.x % nwg, slice = r % nub, mt0 = (r / nub) * MB;
    const LayerDir d = dn ? a.dir[1] : a.dir[0];
    uint4* ring = dn ? x.ring[1] : x.ring[0];
    const int nthr = blockDim.x, nw = nthr >> 6, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int nkb = H / 32, kb0 = wv * KPW, nmt = (B + 15) / 16;
    const size_t slot = (size_t)nmt * 16 * H / 4;      // uint4 per ring slot
    uint4 wh[KPW][NT], wl[KPW][NT];
    {
        const int j = lane & 15, k8 = (lane >> 4) * 8;
#pragma unroll
        for (int kk = 0; kk < KPW; ++kk)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                const int c = nt * 16 + j, g = c / U, u = c % U, k = (kb0 + kk) * 32 + k8;
                const float* src = d.w + (size_t)k * 4 * H + g * H + slice * U + u;
                float v[8];
#pragma unroll
                for (int e = 0; e < 8; ++e) v[e] = src[(size_t)e * 4 * H];
                lbf3_split8(v, wh[kk][nt], wl[kk][nt]);
            }
    }
    const size_t bh = (size_t)B * H;
    for (int s = a.s0; s < a.s1; ++s) {
        if (s > 0 && !layer_wait(d.cnt + s, (unsigned)nwg, a.err, a.limit, &abort_flag)) return;
        f32x4 acc[MB][NT];
        lbf3_product<KPW, MB, NT, PREC>(ring + (s & 1) * slot, nkb, mt0, nmt, kb0, lane, wh, wl, acc);
        lbf3_stage<MB, NT>(red, wv, lane, acc);
        __syncthreads();
        const float* hp = d.hh + (size_t)s * bh;
        unsigned short* hn3 = reinterpret_cast<unsigned short*>(ring + ((s + 1) & 1) * slot);
        for (int cell = threadIdx.x; cell < MB * 16 * U; cell += nthr) {
            const int rl = cell / U, u = cell % U, row = mt0 * 16 + rl, unit = slice * U + u;
            if (row >= B) continue;
            const int len = a.lengths[row];
            const size_t e = ((size_t)s * B + row) * H + unit;
            const float hprev = hp[(size_t)row * H + unit], cprev = d.hc[e];
            float hn = hprev, cn = cprev;
            if (s < len) {
                float p[4];
#pragma unroll
                for (int g = 0; g < 4; ++g) p[g] = lbf3_sum<MB, NT>(red, nw, rl >> 4, rl & 15, g * U + u);
                const float* gg = d.g + ((size_t)s * B + row) * 4 * H + unit;
                const float gi = sigmoidf_(p[0] + gg[0]), gj = tanhf(p[1] + gg[H]);
                const float gf = sigmoidf_(p[2] + gg[2 * H] + a.forget_bias), go = sigmoidf_(p[3] + gg[3 * H]);
                cn = gf * cprev + gi * gj;
                hn = go * tanhf(cn);
                float* ga = d.gates + ((size_t)s * B + row) * 4 * H + unit;
                ga[0] = gi; ga[H] = gj; ga[2 * H] = gf; ga[3 * H] = go;
                const int frame = d.rev ? len - 1 - s : s;
                d.y[((size_t)frame * B + row) * H + unit] = hn * layer_mask(d.seed, 2u * a.layer + 1u, (uint32_t)e, a.keep_out);
            } else {
                d.y[e] = 0.f;
            }
            d.hh[e + bh] = hn;
            d.hc[e + bh] = cn;
            unsigned short hi, lo;
            bf16_split(hn, hi, lo);
            const size_t po = packed_off3(row, unit, H);
            hn3[po] = hi;
            if constexpr (PREC != 2) hn3[po + 512] = lo;
        }
        layer_publish(d.cnt + s + 1);
    }
}

// Backward recurrence of one layer, steps s1-1 down to s0, both directions: grid = ndir x (H / 16) x ngrp workgroups of
// NW = 4H / 32 / KPW waves; dG [T][B][4H] (step order), and its split copy into the ring for the next step.
template <int KPW, int PREC>
__global__ __launch_bounds__(LBF3_BWD_MAXW * 64) void lstm_layer_bwd_bf3(LayerBf3Args x) {
    extern __shared__ float4 lbf3_lds4[];
    float* red = reinterpret_cast<float*>(lbf3_lds4);
    __shared__ int abort_flag;
    constexpr int U = LBF3_BWD_U, NT = LBF3_BWD_NT, MB = LBF3_BWD_MB;
    const LayerArgs& a = x.a;
    const int H = a.H, B = a.B, T = a.T, nub = H / U, nwg = nub * x.ngrp;
    const int dn = blockIdx.x / nwg, r = blockIdx.x % nwg, slice = r % nub, mt0 = (r / nub) * MB;
    const LayerDir d = dn ? a.dir[1] : a.dir[0];
    uint4* ring = dn ? x.ring[1] : x.ring[0];
    const int nthr = blockDim.x, nw = nthr >> 6, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int nkb = 4 * H / 32, kb0 = wv * KPW, nmt = (B + 15) / 16;
    const size_t slot = (size_t)nmt * 16 * 4 * H / 4;
    uint4 wh[KPW][NT], wl[KPW][NT];
    {
        const int j = lane & 15, k8 = (lane >> 4) * 8;       // S[k = c][j] = W_hh[slice * U + j][c]
        int dep = 0;      // (0; the empty asm makes each K-block's loads wait for the previous split: all at once spill at KPW = 16)
#pragma unroll
        for (int kk = 0; kk < KPW; ++kk) {
            const float4* src = reinterpret_cast<const float4*>(d.w + (size_t)(slice * U + j) * 4 * H + (kb0 + kk) * 32 + k8 + dep);
            const float4 v0 = src[0], v1 = src[1];
            const float v[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
            lbf3_split8(v, wh[kk][0], wl[kk][0]);
            asm volatile("" : "+v"(dep) : "v"(wh[kk][0].x), "v"(wl[kk][0].w));
        }
    }
    const size_t bh = (size_t)B * H;
    for (int s = a.s1 - 1; s >= a.s0; --s) {
        const bool has_next = s + 1 < T;
        if (has_next && !layer_wait(d.cnt + s + 1, (unsigned)nwg, a.err, a.limit, &abort_flag)) return;
        f32x4 acc[MB][NT];
        if (has_next) {
            lbf3_product<KPW, MB, NT, PREC>(ring + ((s + 1) & 1) * slot, nkb, mt0, nmt, kb0, lane, wh, wl, acc);
        } else {
#pragma unroll
            for (int m = 0; m < MB; ++m) acc[m][0] = (f32x4){0.f, 0.f, 0.f, 0.f};
        }
        lbf3_stage<MB, NT>(red, wv, lane, acc);
        __syncthreads();
        unsigned short* dg3 = reinterpret_cast<unsigned short*>(ring + (s & 1) * slot);
        for (int cell = threadIdx.x; cell < MB * 16 * U; cell += nthr) {
            const int rl = cell / U, u = cell % U, row = mt0 * 16 + rl, unit = slice * U + u;
            if (row >= B) continue;
            const int len = a.lengths[row];
            const size_t e = ((size_t)s * B + row) * H + unit;
            float* dcp = d.dc + (size_t)row * H + unit;
            float gi = 0.f, gj = 0.f, gf = 0.f, go = 0.f, dcn = 0.f;
            if (s < len) {
                const float p = lbf3_sum<MB, NT>(red, nw, rl >> 4, rl & 15, u);
                const int frame = d.rev ? len - 1 - s : s;
                const float dh = d.dy[((size_t)frame * B + row) * H + unit] *
                                 layer_mask(d.seed, 2u * a.layer + 1u, (uint32_t)e, a.keep_out) + p;
                const float* ga = d.gates + ((size_t)s * B + row) * 4 * H + unit;
                const float i = ga[0], j = ga[H], f = ga[2 * H], o = ga[3 * H];
                const float c = d.hc[e + bh], cprev = d.hc[e];
                const float tc = tanhf(c);
                const float dcv = *dcp + dh * o * (1.f - tc * tc);
                gi = dcv * j * i * (1.f - i);
                gj = dcv * i * (1.f - j * j);
                gf = dcv * cprev * f * (1.f - f);
                go = dh * tc * o * (1.f - o);
                dcn = dcv * f;
            }
            *dcp = dcn;
            float* dgo = d.dg + ((size_t)s * B + row) * 4 * H + unit;
            dgo[0] = gi; dgo[H] = gj; dgo[2 * H] = gf; dgo[3 * H] = go;
            const float gv[4] = {gi, gj, gf, go};
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                unsigned short hi, lo;
                bf16_split(gv[g], hi, lo);
                const size_t po = packed_off3(row, g * H + unit, 4 * H);
                dg3[po] = hi;
                if constexpr (PREC != 2) dg3[po + 512] = lo;
            }
        }
        layer_publish(d.cnt + s);
    }
}
