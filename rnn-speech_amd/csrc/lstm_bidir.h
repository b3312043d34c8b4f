// Layer-wise bidirectional LSTM stacks: the host driver (amdspeech_lstm_bidir_*, include/amdspeech.h).  Included from lstm.hip
// after the kernels it launches (lstm_layer.h, lstm_layer_bf3.h; namespace amdspeech); check_desc, device_cus, the batched
// products (gemm_batched / gemm_reduced) and the profiling hooks come from lstm.hip, pack_rows_bf3_kernel from lstm_step_bf3.h.
//
// Every fwd / bwd call decides its launches ONCE (BidirPlan, built from the descriptor after bidir_check) and launches from the
// struct; amdspeech_lstm_bidir_plan returns the same struct as plain integers.  The size and pointer queries (_workspace_bytes,
// _ws_ptr, _layer_stride, _status) need the layout only and never ask the runtime anything.

struct BidirLayout {
    size_t sync, z0, dz0, g[2], dx[2], dy[2], dc[2], total;
    size_t xin[2], hh[2], hc[2], gates[2], y[2];      // of layer 0; layer l at + l * per_layer[dir]
    size_t per_layer;
    size_t ring[2];       // precision 1 only (behind everything else): the split h / dG ring of each direction
};
static size_t bidir_sync_words(int T) { return 64 + 2 * ((size_t)T + 1); }      // error word, then the two directions' counters
static BidirLayout bidir_layout(const amdspeech_lstm_desc* d) {
    const size_t T = d->T, B = d->B, H = d->H, L = d->L, tbh = T * B * H;
    BidirLayout o;
    size_t off = 0;
    auto take = [&](size_t n) { size_t r = off; off += (n + 63) / 64 * 64; return r; };
    o.sync = take(bidir_sync_words(d->T));      // (first: the block the per-launch memset zeroes)
    o.z0 = take(tbh);
    o.dz0 = take(tbh);
    for (int k = 0; k < 2; ++k) {
        o.g[k] = take(4 * tbh);
        o.dx[k] = take(2 * tbh);
        o.dy[k] = take(tbh);
        o.dc[k] = take(B * H);
    }
    // per layer and direction: the cell input (2H wide: layer 0 uses the first H columns' worth), h / c history, gates, output
    const size_t start = off;
    for (int k = 0; k < 2; ++k) {
        o.xin[k] = take(2 * tbh);
        o.hh[k] = take((T + 1) * B * H);
        o.hc[k] = take((T + 1) * B * H);
        o.gates[k] = take(4 * tbh);
        o.y[k] = take(tbh);
    }
    o.per_layer = off - start;
    off = start + L * o.per_layer;
    o.ring[0] = o.ring[1] = 0;
    if (d->precision == 1)      // two slots of [16 * ceil(B / 16)][4H] (bf16 hi + lo = one float per value); forward uses the first H
        for (int k = 0; k < 2; ++k) o.ring[k] = take(2 * ((B + 15) / 16 * 16) * 4 * H);
    o.total = off;
    return o;
}
static size_t bidir_at(const BidirLayout& o, size_t base, int l) { return base + (size_t)l * o.per_layer; }

// The instantiated bf16x3 recurrence kernels by KPW, the K-blocks (32 wide) a wave takes: what the plan picks from and what
// bidir_lds_attr raises the LDS limit of
struct Bf3Kernel {
    int kpw;
    void (*kern)(LayerBf3Args);
};
static const Bf3Kernel BF3_FWD[] = {{1, lstm_layer_fwd_bf3<1, 1>}, {2, lstm_layer_fwd_bf3<2, 1>}, {4, lstm_layer_fwd_bf3<4, 1>}};
static const Bf3Kernel BF3_BWD[] = {{1, lstm_layer_bwd_bf3<1, 1>}, {2, lstm_layer_bwd_bf3<2, 1>}, {4, lstm_layer_bwd_bf3<4, 1>},
                                    {8, lstm_layer_bwd_bf3<8, 1>}, {16, lstm_layer_bwd_bf3<16, 1>}};
// the first instance whose waves (at most 8 a workgroup) take the whole K (forward K = H, backward K = 4H) between them;
// nullptr = no instance takes this hidden size
template <size_t N>
static const Bf3Kernel* bf3_pick(const Bf3Kernel (&table)[N], int nkb, int max_waves) {
    for (const Bf3Kernel& k : table)
        if (nkb % k.kpw == 0 && nkb / k.kpw <= max_waves) return &k;
    return nullptr;
}
static const Bf3Kernel* bf3_fwd_kernel(const amdspeech_lstm_desc* d) { return bf3_pick(BF3_FWD, d->H / 32, LBF3_FWD_MAXW); }
static const Bf3Kernel* bf3_bwd_kernel(const amdspeech_lstm_desc* d) { return bf3_pick(BF3_BWD, 4 * d->H / 32, LBF3_BWD_MAXW); }

static int bidir_check(const amdspeech_lstm_desc* d) {
    if (int rc = check_desc(d)) return rc;
    if (d->precision == 2) {
        set_error("lstm_bidir: the layer-wise bidirectional mode runs in exact f32 (precision 0) or bf16x3 (1), not plain bf16 (2)");
        return AMDSPEECH_EUNSUPPORTED;
    }
    if (d->precision == 1 && (d->H > 1024 || !bf3_fwd_kernel(d) || !bf3_bwd_kernel(d))) {
        set_error("lstm_bidir: bf16x3 does not take hidden size %d: its kernels split the H (forward) and 4H (backward) rows of "
                  "W_hh over at most 8 waves, 32 x 1, 2, 4, 8 or 16 rows each (H = 64, 128, 256, 512, 768, 1024 qualify)", d->H);
        return AMDSPEECH_EUNSUPPORTED;
    }
    if (d->H > 1024) {
        set_error("lstm_bidir: hidden size %d above 1024 (the recurrence keeps H x %d floats of W_hh per workgroup in LDS)", d->H, 4 * LAYER_U);
        return AMDSPEECH_EUNSUPPORTED;
    }
    AS_CHECK_ARG((size_t)d->T * d->B * 2 * d->H < (1ull << 32), "lstm_bidir: T*B*2H too large for the dropout counter");
    return AMDSPEECH_OK;
}

// The recurrence launch of one pass (forward, backward): kernel, workgroups PER DIRECTION, waves of 64 threads, dynamic LDS (f32: the
// workgroup's slice of W_hh; bf16x3: the partial tiles of every wave), and at bf16x3 the K-blocks per wave and the row groups
struct BidirPass {
    const void* kern;
    int kpw, waves, groups, wgs;
    size_t lds;
};
struct BidirPlan {
    amdspeech_lstm_desc d;
    BidirLayout lo;
    int path;      // 2 = both directions of a layer in ONE persistent launch, 1 = one persistent launch per direction, 0 = one launch per frame
    int cus;
    unsigned long long limit;      // of a bounded wait, 100 MHz ticks (AMDSPEECH_LSTM_INJECT_TIMEOUT: give up at the first unsatisfied one)
    BidirPass pass[2];
    int cell(int k, int l) const { return k * d.L + l; }      // of the 2L cell tensors, the forward cells' layers first
};
static BidirPlan bidir_plan(const amdspeech_lstm_desc* d) {
    static const int env = runtime_switch("AMDSPEECH_BIDIR_PERSISTENT", 1);      // 0: the per-frame launches
    BidirPlan p{};
    p.d = *d;
    p.lo = bidir_layout(d);
    p.cus = device_cus();
    p.limit = (d->flags & AMDSPEECH_LSTM_INJECT_TIMEOUT) ? 0ull : 100000000ull + (unsigned long long)d->T * 10000ull;
    bool persistent = env != 0 && !(d->flags & AMDSPEECH_LSTM_PER_DIAGONAL) && p.cus > 0;
    const int nmt = (d->B + 15) / 16;
    for (int bwd = 0; bwd < 2; ++bwd) {
        BidirPass& q = p.pass[bwd];
        if (d->precision == 1) {
            const Bf3Kernel& k = bwd ? *bf3_bwd_kernel(d) : *bf3_fwd_kernel(d);
            const int mb = bwd ? LBF3_BWD_MB : LBF3_FWD_MB, nt = bwd ? LBF3_BWD_NT : LBF3_FWD_NT, u = bwd ? LBF3_BWD_U : LBF3_FWD_U;
            q.kern = reinterpret_cast<const void*>(k.kern);
            q.kpw = k.kpw;
            q.waves = (bwd ? 4 : 1) * d->H / 32 / k.kpw;
            q.groups = ceil_div(nmt, mb);
            q.wgs = d->H / u * q.groups;
            q.lds = (size_t)q.waves * mb * nt * 1024;
            int per_cu = 0;      // one workgroup per CU, if the kernel's registers and LDS admit one at all
            if (persistent && (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, q.kern, q.waves * 64, q.lds) != hipSuccess || per_cu < 1))
                persistent = false;
        } else {
            q.kern = bwd ? reinterpret_cast<const void*>(lstm_layer_bwd) : reinterpret_cast<const void*>(lstm_layer_fwd);
            q.kpw = 0;
            q.waves = LAYER_THREADS / 64;
            q.groups = 1;
            q.wgs = d->H / LAYER_U;
            q.lds = (size_t)d->H * (bwd ? 4 * LAYER_U : LAYER_FWD_WS) * sizeof(float);
        }
    }
    const int nwg = p.pass[0].wgs > p.pass[1].wgs ? p.pass[0].wgs : p.pass[1].wgs;
    p.path = !persistent ? 0 : 2 * nwg <= p.cus ? 2 : nwg <= p.cus ? 1 : 0;
    return p;
}
static int bidir_lds_attr() {
    static unsigned long long seen = 0;
    if (DeviceOnce once{&seen}) {
        const int max_lds = (int)(1024 * LAYER_FWD_WS * sizeof(float));
        AS_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(lstm_layer_fwd), hipFuncAttributeMaxDynamicSharedMemorySize, max_lds));
        AS_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(lstm_layer_bwd), hipFuncAttributeMaxDynamicSharedMemorySize, max_lds));
        const int max_bf3 = LBF3_FWD_MAXW * LBF3_FWD_MB * LBF3_FWD_NT * 1024;      // (the backward kernels take at most a quarter of it)
        for (const Bf3Kernel& k : BF3_FWD)
            AS_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k.kern), hipFuncAttributeMaxDynamicSharedMemorySize, max_bf3));
        for (const Bf3Kernel& k : BF3_BWD)
            AS_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k.kern), hipFuncAttributeMaxDynamicSharedMemorySize, max_bf3));
        once.done();
    }
    return AMDSPEECH_OK;
}
static uint64_t bidir_seed(const amdspeech_lstm_desc* d, int dir) { return dir ? d->seed ^ 0x5bd1e995ull : d->seed; }

// What both calls check before they plan: the descriptor, the caller's pointers (`ptrs`: all of them given), the workspace's alignment
static int bidir_call_check(const char* fn, const amdspeech_lstm_desc* d, const float* ws, bool ptrs) {
    if (int rc = bidir_check(d)) return rc;
    AS_CHECK_ARG(ws && ptrs, "%s: null pointer", fn);
    AS_CHECK_ARG(((uintptr_t)ws % 256) == 0, "%s: workspace must be 256-byte aligned", fn);
    return AMDSPEECH_OK;
}

// The recurrence arguments of layer l: both directions' cells and the scalars (bidir_recurrence adds the frames [s0, s1) of a launch)
static LayerArgs bidir_layer_args(const BidirPlan& p, float* ws, int l, const float* const* kernels, const int* lengths) {
    const amdspeech_lstm_desc& d = p.d;
    const BidirLayout& lo = p.lo;
    const int W = l ? 2 * d.H : d.H;
    LayerArgs a{};
    for (int k = 0; k < 2; ++k) {
        LayerDir& r = a.dir[k];
        r.g = ws + lo.g[k];
        r.w = kernels[p.cell(k, l)] + (size_t)W * 4 * d.H;
        r.hh = ws + bidir_at(lo, lo.hh[k], l);
        r.hc = ws + bidir_at(lo, lo.hc[k], l);
        r.gates = ws + bidir_at(lo, lo.gates[k], l);
        r.y = ws + bidir_at(lo, lo.y[k], l);
        r.dy = ws + lo.dy[k];
        r.dg = ws + lo.g[k];
        r.dc = ws + lo.dc[k];
        r.cnt = reinterpret_cast<unsigned*>(ws + lo.sync + 64) + (size_t)k * (d.T + 1);
        r.seed = bidir_seed(&d, k);
        r.rev = k;
    }
    a.lengths = lengths; a.T = d.T; a.B = d.B; a.H = d.H; a.layer = l; a.keep_out = d.keep_out; a.forget_bias = 1.0f;
    a.err = reinterpret_cast<unsigned*>(ws + lo.sync);
    a.limit = p.limit;
    return a;
}

// One layer's recurrence (both directions) on the path the plan takes.  The f32 kernels take LayerArgs, the bf16x3 kernels the
// LayerBf3Args that begins with it (then the rings and the row groups): one ladder launches either from the same struct.
static int bidir_recurrence(hipStream_t s, const BidirPlan& p, float* ws, const LayerArgs& a, bool bwd) {
    const BidirPass& q = p.pass[bwd];
    const int T = p.d.T;
    // the counters of both directions (the error word stays: a time-out of an earlier layer is reported, not forgotten)
    AS_CHECK_HIP(hipMemsetAsync(ws + p.lo.sync + 64, 0, 2 * ((size_t)T + 1) * sizeof(unsigned), s));
    LayerBf3Args x{};
    x.a = a;
    x.ngrp = q.groups;
    for (int k = 0; k < 2; ++k) x.ring[k] = reinterpret_cast<uint4*>(ws + p.lo.ring[k]);
    void* args[] = {p.d.precision == 1 ? static_cast<void*>(&x) : static_cast<void*>(&x.a)};
    auto launch = [&](int wgs) { return hipLaunchKernel(q.kern, dim3(wgs), dim3(q.waves * 64), args, q.lds, s); };
    x.a.s0 = 0; x.a.s1 = T;
    if (p.path == 2) {
        AS_CHECK_HIP(launch(2 * q.wgs));
    } else if (p.path == 1) {      // a launch of one direction runs whatever stands first
        AS_CHECK_HIP(launch(q.wgs));
        x.a.dir[0] = a.dir[1];
        x.ring[0] = x.ring[1];
        AS_CHECK_HIP(launch(q.wgs));
    } else {
        for (int t = 0; t < T; ++t) {
            x.a.s0 = bwd ? T - 1 - t : t;
            x.a.s1 = x.a.s0 + 1;
            AS_CHECK_HIP(launch(2 * q.wgs));
        }
    }
    return AMDSPEECH_OK;
}

static int bidir_fwd(hipStream_t s, const amdspeech_lstm_desc* d, float* ws, const float* const* kernels, const float* const* biases,
                     const int* lengths, const float* h0, const float* c0) {
    if (int rc = bidir_call_check("lstm_bidir_fwd", d, ws, kernels && biases && lengths)) return rc;
    for (int i = 0; i < 2 * d->L; ++i) AS_CHECK_ARG(kernels[i] && biases[i], "lstm_bidir_fwd: null kernel / bias of cell %d", i);
    if (int rc = bidir_lds_attr()) return rc;
    const BidirPlan p = bidir_plan(d);
    const BidirLayout& lo = p.lo;
    const int T = d->T, B = d->B, H = d->H;
    const size_t bh = (size_t)B * H;
    AS_CHECK_HIP(hipMemsetAsync(ws + lo.sync, 0, 64 * sizeof(float), s));      // error word
    if (d->precision == 1)      // (the rows of the last 16-row tile past B are read, never written: zero)
        AS_CHECK_HIP(hipMemsetAsync(ws + lo.ring[0], 0, (lo.total - lo.ring[0]) * sizeof(float), s));
    prof_flops(0, 0.0, 0.0);
    prof_begin(0, s);
    for (int l = 0; l < d->L; ++l) {
        const int W = l ? 2 * H : H;
        const float* src0 = l ? ws + bidir_at(lo, lo.y[0], l - 1) : ws + lo.z0;
        const float* src1 = l ? ws + bidir_at(lo, lo.y[1], l - 1) : nullptr;
        for (int k = 0; k < 2; ++k) {
            float* xin = ws + bidir_at(lo, lo.xin[k], l);
            const size_t n4 = (size_t)T * B * W / 4;
            hipLaunchKernelGGL(bidir_pack_kernel, dim3(ceil_div(n4, 256)), dim3(256), 0, s, src0, src1, xin, lengths, T, B, H, W, k,
                               bidir_seed(d, k), l, d->keep_in);
            AS_CHECK_LAUNCH();
            if (int rc = gemm_batched(d, s, false, false, T * B, 4 * H, W, xin, W, kernels[p.cell(k, l)], 4 * H, ws + lo.g[k], 4 * H,
                                      biases[p.cell(k, l)], false))
                return rc;
            float* hh = ws + bidir_at(lo, lo.hh[k], l);
            float* hc = ws + bidir_at(lo, lo.hc[k], l);
            if (k == 0 && h0) AS_CHECK_HIP(hipMemcpyAsync(hh, h0 + l * bh, bh * sizeof(float), hipMemcpyDeviceToDevice, s));
            else AS_CHECK_HIP(hipMemsetAsync(hh, 0, bh * sizeof(float), s));
            if (k == 0 && c0) AS_CHECK_HIP(hipMemcpyAsync(hc, c0 + l * bh, bh * sizeof(float), hipMemcpyDeviceToDevice, s));
            else AS_CHECK_HIP(hipMemsetAsync(hc, 0, bh * sizeof(float), s));
            if (d->precision == 1) {      // the initial h, split, into ring slot 0: what step 0 of the bf16x3 kernel reads
                hipLaunchKernelGGL(pack_rows_bf3_kernel, dim3(ceil_div(bh, 256)), dim3(256), 0, s, hh, bh,
                                   reinterpret_cast<unsigned short*>(ws + lo.ring[k]), B, H, 1);
                AS_CHECK_LAUNCH();
            }
        }
        if (int rc = bidir_recurrence(s, p, ws, bidir_layer_args(p, ws, l, kernels, lengths), false)) return rc;
    }
    prof_end(0, s, p.path ? d->L : d->L * T);
    return AMDSPEECH_OK;
}

static int bidir_bwd(hipStream_t s, const amdspeech_lstm_desc* d, float* ws, const float* const* kernels, float* const* dkernels,
                     float* const* dbiases, const int* lengths) {
    if (int rc = bidir_call_check("lstm_bidir_bwd", d, ws, kernels && dkernels && dbiases && lengths)) return rc;
    for (int i = 0; i < 2 * d->L; ++i) AS_CHECK_ARG(kernels[i] && dkernels[i] && dbiases[i], "lstm_bidir_bwd: null pointer of cell %d", i);
    if (int rc = bidir_lds_attr()) return rc;
    const BidirPlan p = bidir_plan(d);
    const BidirLayout& lo = p.lo;
    const int T = d->T, B = d->B, H = d->H, TB = T * B;
    if (d->precision == 1)      // (the error word is left alone: a time-out of the forward call stays reported)
        AS_CHECK_HIP(hipMemsetAsync(ws + lo.ring[0], 0, (lo.total - lo.ring[0]) * sizeof(float), s));
    prof_flops(1, 0.0, 0.0);
    prof_begin(1, s);
    for (int l = d->L - 1; l >= 0; --l) {
        const int W = l ? 2 * H : H;
        for (int k = 0; k < 2; ++k) AS_CHECK_HIP(hipMemsetAsync(ws + lo.dc[k], 0, (size_t)B * H * sizeof(float), s));
        if (int rc = bidir_recurrence(s, p, ws, bidir_layer_args(p, ws, l, kernels, lengths), true)) return rc;
        for (int k = 0; k < 2; ++k) {
            const float* dG = ws + lo.g[k];
            float* dK = dkernels[p.cell(k, l)];
            // dK[0:W] += X^T . dG (+ db), dK[W:W+H] += Hprev^T . dG, dX = dG . W_ih^T
            const float* X = ws + bidir_at(lo, lo.xin[k], l);
            if (d->precision == 0) {
                if (int rc = gemm_f32(s, true, false, W, 4 * H, TB, X, W, dG, 4 * H, dK, 4 * H, nullptr, true, dbiases[p.cell(k, l)])) return rc;
            } else {
                if (int rc = gemm_reduced(d, s, true, false, W, 4 * H, TB, X, W, dG, 4 * H, dK, 4 * H, nullptr, true)) return rc;
                if (int rc = colsum_accumulate(s, dG, TB, 4 * H, 4 * H, dbiases[p.cell(k, l)])) return rc;
            }
            if (int rc = gemm_batched(d, s, true, false, H, 4 * H, TB, ws + bidir_at(lo, lo.hh[k], l), H, dG, 4 * H, dK + (size_t)W * 4 * H,
                                      4 * H, nullptr, true)) return rc;
            if (int rc = gemm_batched(d, s, false, true, TB, W, 4 * H, dG, 4 * H, kernels[p.cell(k, l)], 4 * H, ws + lo.dx[k], W, nullptr, false))
                return rc;
        }
        const size_t n4 = (size_t)T * B * W / 4;
        float* out0 = l ? ws + lo.dy[0] : ws + lo.dz0;
        float* out1 = l ? ws + lo.dy[1] : nullptr;
        hipLaunchKernelGGL(bidir_split_kernel, dim3(ceil_div(n4, 256)), dim3(256), 0, s, ws + lo.dx[0], ws + lo.dx[1], out0, out1, lengths,
                           T, B, H, W, bidir_seed(d, 0), bidir_seed(d, 1), l, d->keep_in);
        AS_CHECK_LAUNCH();
    }
    prof_end(1, s, p.path ? d->L : d->L * T);
    return AMDSPEECH_OK;
}

extern "C" size_t amdspeech_lstm_bidir_workspace_bytes(const amdspeech_lstm_desc* d) {
    if (bidir_check(d) != AMDSPEECH_OK) return 0;
    return bidir_layout(d).total * sizeof(float);
}
extern "C" void* amdspeech_lstm_bidir_ws_ptr(const amdspeech_lstm_desc* d, void* ws, int which) {
    if (ws == nullptr || bidir_check(d) != AMDSPEECH_OK) return nullptr;
    const BidirLayout lo = bidir_layout(d);
    float* w = static_cast<float*>(ws);
    const size_t T = d->T, bh = (size_t)d->B * d->H;
    switch (which) {
        case AMDSPEECH_BIDIR_WS_Z0: return w + lo.z0;
        case AMDSPEECH_BIDIR_WS_YTOP_FW: return w + bidir_at(lo, lo.y[0], d->L - 1);
        case AMDSPEECH_BIDIR_WS_YTOP_BW: return w + bidir_at(lo, lo.y[1], d->L - 1);
        case AMDSPEECH_BIDIR_WS_DYTOP_FW: return w + lo.dy[0];
        case AMDSPEECH_BIDIR_WS_DYTOP_BW: return w + lo.dy[1];
        case AMDSPEECH_BIDIR_WS_DZ0: return w + lo.dz0;
        case AMDSPEECH_BIDIR_WS_HFINAL: return w + lo.hh[0] + T * bh;
        case AMDSPEECH_BIDIR_WS_CFINAL: return w + lo.hc[0] + T * bh;
        default: set_error("lstm_bidir_ws_ptr: unknown region %d", which); return nullptr;
    }
}
extern "C" long amdspeech_lstm_bidir_layer_stride(const amdspeech_lstm_desc* d) {
    if (bidir_check(d) != AMDSPEECH_OK) return -1;
    return (long)bidir_layout(d).per_layer;
}
// The plan as plain numbers (amdspeech.h: amdspeech_lstm_bidir_plan_info): reads bidir_plan, decides nothing
extern "C" int amdspeech_lstm_bidir_plan(const amdspeech_lstm_desc* d, amdspeech_lstm_bidir_plan_info* out) {
    if (int rc = bidir_check(d)) return rc;
    AS_CHECK_ARG(out != nullptr, "lstm_bidir_plan: null output");
    const BidirPlan p = bidir_plan(d);
    const BidirPass &f = p.pass[0], &b = p.pass[1];
    *out = amdspeech_lstm_bidir_plan_info{p.path, p.cus, f.kpw, f.waves, f.groups, f.wgs, (int)f.lds, b.kpw, b.waves, b.groups, b.wgs, (int)b.lds};
    return AMDSPEECH_OK;
}
extern "C" int amdspeech_lstm_bidir_path(const amdspeech_lstm_desc* d) {
    if (int rc = bidir_check(d)) return rc;
    return bidir_plan(d).path;
}
extern "C" int amdspeech_lstm_bidir_fwd(void* stream, const amdspeech_lstm_desc* d, void* ws, const float* const* kernels,
                                        const float* const* biases, const int* lengths, const float* h0, const float* c0) {
    return bidir_fwd(static_cast<hipStream_t>(stream), d, static_cast<float*>(ws), kernels, biases, lengths, h0, c0);
}
extern "C" int amdspeech_lstm_bidir_bwd(void* stream, const amdspeech_lstm_desc* d, void* ws, const float* const* kernels,
                                        float* const* dkernels, float* const* dbiases, const int* lengths) {
    return bidir_bwd(static_cast<hipStream_t>(stream), d, static_cast<float*>(ws), kernels, dkernels, dbiases, lengths);
}
extern "C" int amdspeech_lstm_bidir_status(const amdspeech_lstm_desc* d, void* ws) {
    if (int rc = bidir_check(d)) return rc;
    AS_CHECK_ARG(ws != nullptr, "lstm_bidir_status: null workspace");
    unsigned err = 0;
    AS_CHECK_HIP(hipMemcpy(&err, static_cast<float*>(ws) + bidir_layout(d).sync, sizeof(err), hipMemcpyDeviceToHost));
    if (err != 0) {
        set_error("lstm_bidir: a bounded wait of the persistent per-layer kernels timed out (the workgroups of one launch were not "
                  "all resident); results of this step are invalid -- repeat it with AMDSPEECH_LSTM_PER_DIAGONAL");
        return AMDSPEECH_ETIMEOUT;
    }
    return AMDSPEECH_OK;
}
extern "C" int amdspeech_lstm_bidir_dropout_multipliers(void* stream, const amdspeech_lstm_desc* d, int dir, int which, int layer,
                                                        float* out) {
    if (int rc = bidir_check(d)) return rc;
    AS_CHECK_ARG(out != nullptr && (dir == 0 || dir == 1) && (which == 0 || which == 1) && layer >= 0 && layer < d->L,
                 "lstm_bidir_dropout_multipliers: dir 0 / 1, which 0 (input mask) / 1 (output mask), layer in [0, L)");
    const int W = which == 1 ? d->H : (layer ? 2 * d->H : d->H);
    const size_t n = (size_t)d->T * d->B * W;
    hipLaunchKernelGGL(bidir_mask_kernel, dim3(ceil_div(n, 256)), dim3(256), 0, static_cast<hipStream_t>(stream), out, n,
                       bidir_seed(d, dir), (uint32_t)(2 * layer + which), which ? d->keep_out : d->keep_in);
    AS_CHECK_LAUNCH();
    return AMDSPEECH_OK;
}
