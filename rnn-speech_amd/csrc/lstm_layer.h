// Layer-wise bidirectional LSTM stacks (tf.contrib.rnn.stack_bidirectional_dynamic_rnn, torch.nn.LSTM(bidirectional=True)):
// the per-layer recurrence kernels and the pack / split kernels between layers.  Included from lstm.hip (namespace amdspeech);
// the host driver is amdspeech_lstm_bidir_fwd / _bwd there.
//
// Layer l of either direction reads its whole input before it starts (layer 0: Z_0; above: [h_fw ; h_bw] of layer l-1), so the
// stack runs layer by layer: pack the input of both directions (dropout mask applied, the backward direction reversed by row
// length), ONE batched product G = X . W_ih + b per direction (gemm_f32), then ONE persistent launch that runs the recurrence of
// BOTH directions (one half of the workgroups each).  Everything a recurrence kernel keeps is in STEP order (step s of the
// backward direction is frame len_b - 1 - s of row b); only the layer outputs y / their gradients dy are in forward time, and the
// `rev` flag of a direction makes the kernel read / write those at the reversed frame.
//
// Recurrence kernels: a workgroup owns LAYER_U hidden units x 4 gates of one direction for every batch row and keeps its slice of
// W_hh in LDS for the whole sequence (H x 4U floats forward, 4H x U backward: 128 KiB at H = 1024).  Per step it reads the full
// h_{s-1} (forward) or dG_{s+1} (backward) panel that all workgroups of its direction wrote one step earlier, multiplies by its
// slice on the vector ALUs (exact f32), applies the cell, and publishes its part.  Hand-off between steps: the agent-scope
// release / acquire counter protocol (every wave drains its stores, barrier, ONE lane fences and adds to the step's counter;
// the consumer polls the counter relaxed, then ONE agent acquire), bounded by a wall-clock limit that ends the launch and sets
// the error word amdspeech_lstm_bidir_status reports as AMDSPEECH_ETIMEOUT.  The per-frame fallback launches the SAME kernel for
// one step at a time: the counters it waits for were completed by the previous launch, so no workgroup ever waits for another
// of its own launch -- same arithmetic, same results, no co-residency requirement.

constexpr int LAYER_U = 8;            // hidden units per workgroup (x 4 gates)
constexpr int LAYER_THREADS = 512;    // 8 waves; a wave covers 8 batch rows (4 row pairs x 16 K slices)
constexpr int LAYER_ROWS = 64;        // batch rows per pass of the workgroup
constexpr int LAYER_FWD_WS = 4 * LAYER_U + 4;      // LDS row stride of the forward slice (floats; padded against bank conflicts)

struct LayerDir {
    const float* g;       // forward: [T][B][4H] x . W_ih + b (step order)
    const float* w;       // W_hh [H][4H] (the h rows of the TF kernel)
    float* hh;            // [T+1][B][H] h, step order, slot 0 = initial state
    float* hc;            // [T+1][B][H] c
    float* gates;         // [T][B][4H] activated i, j, f, o (step order)
    float* y;             // forward out: [T][B][H] forward time, output dropout applied, 0 past the length
    const float* dy;      // backward in: [T][B][H] forward time (gradient of y)
    float* dg;            // backward out: [T][B][4H] gate pre-activation gradients (step order)
    float* dc;            // backward: [B][H] carried cell-state gradient
    unsigned* cnt;        // [T+1] workgroups that have published a slot
    uint64_t seed;        // the direction's dropout stream
    int rev;
};
struct LayerArgs {
    LayerDir dir[2];
    const int* lengths;
    unsigned* err;        // error word: nonzero = a bounded wait gave up
    int T, B, H, layer, s0, s1;
    float keep_out, forget_bias;
    unsigned long long limit;      // 100 MHz ticks
};

typedef __attribute__((address_space(1))) unsigned gu32_t;

__device__ __forceinline__ float layer_mask(uint64_t seed, uint32_t stream, uint32_t idx, float keep) {
    if (keep >= 1.0f) return 1.0f;
    return uniform01(seed, stream, idx) < keep ? 1.0f / keep : 0.0f;
}

// every thread: wait until `*cnt` reaches `need` (thread 0 polls), then the agent-scope acquire; false = give up (timed out, or
// another workgroup did)
__device__ __forceinline__ bool layer_wait(unsigned* cnt, unsigned need, unsigned* err, unsigned long long limit, int* abort_flag) {
    if (threadIdx.x == 0) {
        gu32_t* c = (gu32_t*)cnt;
        gu32_t* e = (gu32_t*)err;
        int ab = 0;
        if (__hip_atomic_load(c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < need) {
            const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
            for (unsigned spins = 0;; ++spins) {
                if (__hip_atomic_load(c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= need) break;
                if ((spins & 31) == 0 && (__hip_atomic_load(e, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u ||
                                          __builtin_amdgcn_s_memrealtime() - t0 >= limit)) {
                    ab = 1;
                    break;
                }
                __builtin_amdgcn_s_sleep(1);
            }
        }
        if (ab) __hip_atomic_fetch_or(e, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        *abort_flag = ab;
    }
    __syncthreads();
    return *abort_flag == 0;
}
// every thread, after its stores of a slot: drain, barrier, ONE lane releases at agent scope and counts the workgroup in
__device__ __forceinline__ void layer_publish(unsigned* cnt) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __hip_atomic_fetch_add((gu32_t*)cnt, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// Forward recurrence of one layer, steps [s0, s1), both directions (grid = ndir * H / LAYER_U workgroups).
__global__ __launch_bounds__(LAYER_THREADS) void lstm_layer_fwd(LayerArgs a) {
    extern __shared__ float4 layer_lds4[];
    float* wl = reinterpret_cast<float*>(layer_lds4);
    __shared__ int abort_flag;
    constexpr int U = LAYER_U;
    const int H = a.H, B = a.B, nwg = H / U;
    const int dn = blockIdx.x / nwg, slice = blockIdx.x % nwg;
    const LayerDir d = dn ? a.dir[1] : a.dir[0];
    for (int e = threadIdx.x; e < H * 4 * U; e += LAYER_THREADS) {
        const int k = e / (4 * U), c = e % (4 * U), g = c / U, u = c % U;
        wl[k * LAYER_FWD_WS + c] = d.w[(size_t)k * 4 * H + g * H + slice * U + u];
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, ks = lane & 15, rp = lane >> 4;
    const int rr = ks & 1, u = ks >> 1, unit = slice * U + u;
    const size_t bh = (size_t)B * H;
    for (int s = a.s0; s < a.s1; ++s) {
        if (s > 0 && !layer_wait(d.cnt + s, (unsigned)nwg, a.err, a.limit, &abort_flag)) return;
        const float* hp = d.hh + (size_t)s * bh;
        for (int rb = 0; rb < B; rb += LAYER_ROWS) {
            const int r0 = rb + (wv * 4 + rp) * 2;
            const bool v0 = r0 < B, v1 = r0 + 1 < B;
            float acc0[4 * U], acc1[4 * U];
#pragma unroll
            for (int c = 0; c < 4 * U; ++c) acc0[c] = acc1[c] = 0.f;
            for (int k = ks; k < H; k += 16) {
                const float h0 = v0 ? hp[(size_t)r0 * H + k] : 0.f;
                const float h1 = v1 ? hp[(size_t)(r0 + 1) * H + k] : 0.f;
                const float4* wr = reinterpret_cast<const float4*>(wl + k * LAYER_FWD_WS);
#pragma unroll
                for (int q = 0; q < U; ++q) {
                    const float4 w4 = wr[q];
                    acc0[4 * q] += h0 * w4.x; acc0[4 * q + 1] += h0 * w4.y; acc0[4 * q + 2] += h0 * w4.z; acc0[4 * q + 3] += h0 * w4.w;
                    acc1[4 * q] += h1 * w4.x; acc1[4 * q + 1] += h1 * w4.y; acc1[4 * q + 2] += h1 * w4.z; acc1[4 * q + 3] += h1 * w4.w;
                }
            }
#pragma unroll
            for (int c = 0; c < 4 * U; ++c)
#pragma unroll
                for (int off = 1; off < 16; off <<= 1) {
                    acc0[c] += __shfl_xor(acc0[c], off);
                    acc1[c] += __shfl_xor(acc1[c], off);
                }
            float p[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int uu = 0; uu < U; ++uu)
                if (uu == u) {
#pragma unroll
                    for (int g = 0; g < 4; ++g) p[g] = rr ? acc1[g * U + uu] : acc0[g * U + uu];
                }
            const int row = r0 + rr;
            if (row < B) {
                const int len = a.lengths[row];
                const size_t e = ((size_t)s * B + row) * H + unit;
                const float hprev = hp[(size_t)row * H + unit], cprev = d.hc[e];
                float hn = hprev, cn = cprev;
                if (s < len) {
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
                    d.y[e] = 0.f;      // (frames past the length: no step of either direction writes them otherwise)
                }
                d.hh[e + bh] = hn;
                d.hc[e + bh] = cn;
            }
        }
        layer_publish(d.cnt + s + 1);
    }
}

// Backward recurrence of one layer, steps s1-1 down to s0, both directions: dG [T][B][4H] (step order).
__global__ __launch_bounds__(LAYER_THREADS) void lstm_layer_bwd(LayerArgs a) {
    extern __shared__ float4 layer_lds4[];
    float* wt = reinterpret_cast<float*>(layer_lds4);
    __shared__ int abort_flag;
    constexpr int U = LAYER_U;
    const int H = a.H, B = a.B, T = a.T, nwg = H / U;
    const int dn = blockIdx.x / nwg, slice = blockIdx.x % nwg;
    const LayerDir d = dn ? a.dir[1] : a.dir[0];
    for (int e = threadIdx.x; e < H * 4 * U; e += LAYER_THREADS) {      // wt[c][u] = W_hh[slice*U + u][c]
        const int c = e / U, uu = e % U;
        wt[e] = d.w[(size_t)(slice * U + uu) * 4 * H + c];
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, ks = lane & 15, rp = lane >> 4;
    const int rr = ks & 1, u = ks >> 1, unit = slice * U + u;
    const size_t bh = (size_t)B * H, bg = (size_t)B * 4 * H;
    for (int s = a.s1 - 1; s >= a.s0; --s) {
        const bool has_next = s + 1 < T;
        if (has_next && !layer_wait(d.cnt + s + 1, (unsigned)nwg, a.err, a.limit, &abort_flag)) return;
        const float* dgn = d.dg + (size_t)(s + 1) * bg;
        for (int rb = 0; rb < B; rb += LAYER_ROWS) {
            const int r0 = rb + (wv * 4 + rp) * 2;
            const bool v0 = r0 < B, v1 = r0 + 1 < B;
            float acc0[U], acc1[U];
#pragma unroll
            for (int c = 0; c < U; ++c) acc0[c] = acc1[c] = 0.f;
            if (has_next)
                for (int c = ks; c < 4 * H; c += 16) {
                    const float d0 = v0 ? dgn[(size_t)r0 * 4 * H + c] : 0.f;
                    const float d1 = v1 ? dgn[(size_t)(r0 + 1) * 4 * H + c] : 0.f;
                    const float4* wr = reinterpret_cast<const float4*>(wt + c * U);
#pragma unroll
                    for (int q = 0; q < U / 4; ++q) {
                        const float4 w4 = wr[q];
                        acc0[4 * q] += d0 * w4.x; acc0[4 * q + 1] += d0 * w4.y; acc0[4 * q + 2] += d0 * w4.z; acc0[4 * q + 3] += d0 * w4.w;
                        acc1[4 * q] += d1 * w4.x; acc1[4 * q + 1] += d1 * w4.y; acc1[4 * q + 2] += d1 * w4.z; acc1[4 * q + 3] += d1 * w4.w;
                    }
                }
#pragma unroll
            for (int c = 0; c < U; ++c)
#pragma unroll
                for (int off = 1; off < 16; off <<= 1) {
                    acc0[c] += __shfl_xor(acc0[c], off);
                    acc1[c] += __shfl_xor(acc1[c], off);
                }
            float p = 0.f;
#pragma unroll
            for (int uu = 0; uu < U; ++uu)
                if (uu == u) p = rr ? acc1[uu] : acc0[uu];
            const int row = r0 + rr;
            if (row < B) {
                const int len = a.lengths[row];
                const size_t e = ((size_t)s * B + row) * H + unit;
                float* dcp = d.dc + (size_t)row * H + unit;
                float gi = 0.f, gj = 0.f, gf = 0.f, go = 0.f, dcn = 0.f;
                if (s < len) {
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
            }
        }
        layer_publish(d.cnt + s);
    }
}

// The input of one direction's cell at layer l, step order: xin[s][b][k] = in[frame][b][k] x input-dropout multiplier, frame = s
// (forward) or len_b - 1 - s (backward), 0 for s >= len_b.  in = Z_0 (W = H) or [y_fw ; y_bw] of layer l-1 (W = 2H).
__global__ __launch_bounds__(256) void bidir_pack_kernel(const float* __restrict__ src0, const float* __restrict__ src1,
                                                         float* __restrict__ xin, const int* __restrict__ lengths, int T, int B,
                                                         int H, int W, int rev, uint64_t seed, int layer, float keep_in) {
    const size_t per4 = (size_t)B * W / 4;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= per4 * T) return;
    const int s = i / per4;
    const size_t r = (i % per4) * 4;
    const int b = r / W, k = r % W;
    const int len = lengths[b];
    const size_t e = (size_t)s * B * W + r;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (s < len) {
        const int frame = rev ? len - 1 - s : s;
        const float* src = k < H ? src0 + ((size_t)frame * B + b) * H + k : src1 + ((size_t)frame * B + b) * H + (k - H);
        v = *reinterpret_cast<const float4*>(src);
        if (keep_in < 1.0f) {
            v.x *= layer_mask(seed, 2u * layer, (uint32_t)e, keep_in);
            v.y *= layer_mask(seed, 2u * layer, (uint32_t)(e + 1), keep_in);
            v.z *= layer_mask(seed, 2u * layer, (uint32_t)(e + 2), keep_in);
            v.w *= layer_mask(seed, 2u * layer, (uint32_t)(e + 3), keep_in);
        }
    }
    *reinterpret_cast<float4*>(xin + e) = v;
}

// The inverse: the two directions' input gradients dX [T][B][W] (step order) of layer l -> the gradient of layer l-1's outputs
// (forward time): out0 = columns [0, H) (dy_fw, or dZ_0 at l = 0), out1 = columns [H, 2H) (dy_bw).  Each direction's input
// dropout mask is applied; the backward direction's rows are un-reversed and added in.
__global__ __launch_bounds__(256) void bidir_split_kernel(const float* __restrict__ dxf, const float* __restrict__ dxb,
                                                          float* __restrict__ out0, float* __restrict__ out1,
                                                          const int* __restrict__ lengths, int T, int B, int H, int W,
                                                          uint64_t seed_f, uint64_t seed_b, int layer, float keep_in) {
    const size_t per4 = (size_t)B * W / 4;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= per4 * T) return;
    const int t = i / per4;
    const size_t r = (i % per4) * 4;
    const int b = r / W, k = r % W;
    const int len = lengths[b];
    const size_t ef = (size_t)t * B * W + r;
    float4 v = *reinterpret_cast<const float4*>(dxf + ef);
    if (keep_in < 1.0f) {
        v.x *= layer_mask(seed_f, 2u * layer, (uint32_t)ef, keep_in);
        v.y *= layer_mask(seed_f, 2u * layer, (uint32_t)(ef + 1), keep_in);
        v.z *= layer_mask(seed_f, 2u * layer, (uint32_t)(ef + 2), keep_in);
        v.w *= layer_mask(seed_f, 2u * layer, (uint32_t)(ef + 3), keep_in);
    }
    if (t < len) {
        const size_t eb = (size_t)(len - 1 - t) * B * W + r;
        float4 q = *reinterpret_cast<const float4*>(dxb + eb);
        if (keep_in < 1.0f) {
            q.x *= layer_mask(seed_b, 2u * layer, (uint32_t)eb, keep_in);
            q.y *= layer_mask(seed_b, 2u * layer, (uint32_t)(eb + 1), keep_in);
            q.z *= layer_mask(seed_b, 2u * layer, (uint32_t)(eb + 2), keep_in);
            q.w *= layer_mask(seed_b, 2u * layer, (uint32_t)(eb + 3), keep_in);
        }
        v.x += q.x; v.y += q.y; v.z += q.z; v.w += q.w;
    }
    float* o = k < H ? out0 + ((size_t)t * B + b) * H + k : out1 + ((size_t)t * B + b) * H + (k - H);
    *reinterpret_cast<float4*>(o) = v;
}

// The dropout multipliers one direction's cell applies (export for a checker): which = 0 its input mask [T][B][W] (step order),
// which = 1 its output mask [T][B][H] (step order)
__global__ void bidir_mask_kernel(float* out, size_t n, uint64_t seed, uint32_t stream, float keep) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = layer_mask(seed, stream, (uint32_t)i, keep);
}
