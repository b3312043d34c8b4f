// The two ends of a character language-model step that are not CTC-shaped (amdspeech.h: "Language model"): the token lookup in
// front of the LSTM stack and the softmax cross-entropy behind the output Linear.  No reference counterpart in this form: the
// reference's LanguageModel feeds one-hot rows through the input Linear and trains with CTC on shifted labels.
//
//   tokens: int32 [B][ld] row-major, ld >= T; position (t, b) reads ids[b * ld + t]; lengths int32 [B], all on the DEVICE.
//
//   embed_fwd   out[t][b][:] = w[id][:] + bias   where t < lengths[b] and 0 <= id < V, bias elsewhere (a zero one-hot row)
//   embed_bwd   dw[v][:] += sum of dz[t][b][:] over the live positions holding v;  dbias += sum over all t < lengths[b]
//   xent        nll[t][b] = logsumexp(row) - row[target];  dlogits = scale * (softmax(row) - onehot);  loss[b] = sum_t nll
//
// All three are bandwidth-bound and hold no state: plain loads and stores, wave64 shuffles for the row reductions, no atomics,
// no inline assembly, every loop bounded by the shape.
#include "common.h"

#include <math.h>

namespace amdspeech {

constexpr int EMB_THREADS = 256;
constexpr int EMB_MAX_WGS = 4096;          // embed_fwd streams: cap the grid and stride the rest
constexpr int EMB_SEG = 32;                // embed_bwd: positions per segment (one partial row per distinct token and segment)
constexpr int EMB_SUM_CHUNK = 16384;       // embed_bwd, second pass: slots scanned between two barriers (one mask bit each in LDS)
constexpr int EMB_SUM_SCAN = 2048;         // ... slot words loaded together while scanning
constexpr int EMB_SUM_BATCH = 32;          // ... and partial rows loaded before they are added

// ------------------------------------------------------------------------------------------------------------ embed_fwd
// One thread per 16-byte word of out; a row of w is read by H/4 consecutive lanes (whole 64-byte lines for H >= 16).
__global__ __launch_bounds__(EMB_THREADS) void embed_fwd_kernel(const int* __restrict__ ids, int ld, const int* __restrict__ lengths,
                                                                int B, int V, int hv, long n_words, const f32x4* __restrict__ w,
                                                                const f32x4* __restrict__ bias, f32x4* __restrict__ out) {
    for (long i = (long)blockIdx.x * EMB_THREADS + threadIdx.x; i < n_words; i += (long)gridDim.x * EMB_THREADS) {
        const long p = i / hv;
        const int col = (int)(i - p * hv);
        const int t = (int)(p / B), b = (int)(p - (long)t * B);
        f32x4 v = {0.0f, 0.0f, 0.0f, 0.0f};
        if (bias) v = bias[col];
        if (t < lengths[b]) {
            const int id = ids[(long)b * ld + t];
            if (id >= 0 && id < V) {
                const f32x4 r = w[(long)id * hv + col];
                v = bias ? r + v : r;      // (one rounding of w + bias; without a bias the row's own bits)
            }
        }
        out[i] = v;
    }
}

// ------------------------------------------------------------------------------------------------------------ embed_bwd
// A scatter-add without atomics and with a fixed order.  The T * B positions p = t * B + b are cut into segments of EMB_SEG.
//   pass 1 (one workgroup per segment and column block): the first position of each token in the segment -- its "leader" --
//       sums the rows of all positions of the segment that hold the same token, in increasing p, into partial[leader p][:];
//       slot_tok[p] = the token where p is a leader, -1 elsewhere.  The rows of all live positions go into bias_part[seg][:].
//   pass 2 (one workgroup per token and column block): the leaders of token v are found with one ballot per 64 slots and their
//       partial rows are added in increasing p, then dw[v] += that sum.  A token without a leader is not written at all.
// Every position of the text holding ONE token still gives T * B / EMB_SEG leaders that pass 1 sums in parallel; pass 2 then adds
// that many rows for the one token (322 at 161 x 64), and nothing else anywhere.
struct EmbBwdLayout {
    int n_seg;
    long n_slots;          // n_seg * EMB_SEG
    size_t slot_tok, seg_live, bias_part, partial, total;      // byte offsets
};

static EmbBwdLayout emb_bwd_layout(int T, int B, int H) {
    EmbBwdLayout l;
    const long n = (long)T * B;
    l.n_seg = (int)((n + EMB_SEG - 1) / EMB_SEG);
    l.n_slots = (long)l.n_seg * EMB_SEG;
    l.slot_tok = 0;
    l.seg_live = align_up((size_t)l.n_slots * 4, 256);
    l.bias_part = align_up(l.seg_live + (size_t)l.n_seg * 4, 256);
    l.partial = align_up(l.bias_part + (size_t)l.n_seg * H * 4, 256);
    l.total = l.partial + (size_t)l.n_slots * H * 4;
    return l;
}

static int emb_threads(int hv) { return hv <= 64 ? 64 : hv <= 128 ? 128 : 256; }

constexpr int EMB_DEAD = -2, EMB_NO_ROW = -1;      // a position past its row's length; a live position whose id is outside 0 .. V-1

__global__ __launch_bounds__(EMB_THREADS) void embed_bwd_partial_kernel(const int* __restrict__ ids, int ld, const int* __restrict__ lengths,
                                                                        long n_pos, int B, int V, int hv, const f32x4* __restrict__ dz,
                                                                        int* __restrict__ slot_tok, int* __restrict__ seg_live,
                                                                        f32x4* __restrict__ bias_part, f32x4* __restrict__ partial) {
    __shared__ int tok[EMB_SEG];
    __shared__ int lead[EMB_SEG];
    const int seg = blockIdx.x, tid = threadIdx.x;
    const long p0 = (long)seg * EMB_SEG;
    if (tid < EMB_SEG) {
        const long p = p0 + tid;
        int tk = EMB_DEAD;
        if (p < n_pos) {
            const int t = (int)(p / B), b = (int)(p - (long)t * B);
            if (t < lengths[b]) {
                const int id = ids[(long)b * ld + t];
                tk = id >= 0 && id < V ? id : EMB_NO_ROW;
            }
        }
        tok[tid] = tk;
    }
    __syncthreads();
    if (tid < EMB_SEG) {
        const int tk = tok[tid];
        int l = tk >= 0;
        for (int k = 0; k < tid; ++k) l &= tok[k] != tk;
        lead[tid] = l;
        if (blockIdx.y == 0) slot_tok[p0 + tid] = l ? tk : -1;
    }
    if (tid == 0 && blockIdx.y == 0) {
        int live = 0;
        for (int k = 0; k < EMB_SEG; ++k) live |= tok[k] != EMB_DEAD;
        seg_live[seg] = live;
    }
    __syncthreads();
    const int col = blockIdx.y * blockDim.x + tid;
    if (col >= hv) return;
    const f32x4* rows = dz + p0 * hv + col;
    // the segment's rows into registers first: EMB_SEG independent 16-byte loads in flight, then sums in position order
    f32x4 r[EMB_SEG];
#pragma unroll
    for (int j = 0; j < EMB_SEG; ++j) {
        r[j] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        if (tok[j] != EMB_DEAD) r[j] = rows[(long)j * hv];
    }
    if (bias_part) {
        f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int j = 0; j < EMB_SEG; ++j)
            if (tok[j] != EMB_DEAD) acc += r[j];
        bias_part[(long)seg * hv + col] = acc;
    }
#pragma unroll
    for (int j = 0; j < EMB_SEG; ++j) {
        if (!lead[j]) continue;                    // (uniform over the workgroup)
        const int tk = tok[j];
        f32x4 acc = r[j];
#pragma unroll
        for (int k = j + 1; k < EMB_SEG; ++k)
            if (tok[k] == tk) acc += r[k];
        partial[(p0 + j) * hv + col] = acc;
    }
}

__global__ __launch_bounds__(EMB_THREADS) void embed_bwd_sum_kernel(int V, int hv, int n_seg, long n_slots, const int* __restrict__ slot_tok,
                                                                    const int* __restrict__ seg_live, const f32x4* __restrict__ bias_part,
                                                                    const f32x4* __restrict__ partial, f32x4* __restrict__ dw,
                                                                    f32x4* __restrict__ dbias) {
    __shared__ unsigned long long masks[EMB_SUM_CHUNK / 64];
    const int v = blockIdx.x, tid = threadIdx.x;
    const int col = blockIdx.y * blockDim.x + tid;
    const bool own = col < hv;
    f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
    bool any = false;
    if (v == V) {                                  // the bias: the segments' sums in segment order
        if (!dbias || !own) return;
        for (int s0 = 0; s0 < n_seg; s0 += EMB_SUM_BATCH) {      // EMB_SUM_BATCH loads in flight, added in segment order
            f32x4 r[EMB_SUM_BATCH];
            bool on[EMB_SUM_BATCH];
#pragma unroll
            for (int i = 0; i < EMB_SUM_BATCH; ++i) {
                on[i] = s0 + i < n_seg && seg_live[s0 + i] != 0;
                if (on[i]) r[i] = bias_part[(long)(s0 + i) * hv + col];
            }
#pragma unroll
            for (int i = 0; i < EMB_SUM_BATCH; ++i)
                if (on[i]) { acc += r[i]; any = true; }
        }
        if (any) dbias[col] += acc;
        return;
    }
    // EMB_SUM_CHUNK slots at a time: one ballot per 64 slots into LDS, then the token's partial rows of the chunk in slot order,
    // EMB_SUM_BATCH loads in flight before their adds (the order of the adds is the slot order all the same)
    for (long base = 0; base < n_slots; base += EMB_SUM_CHUNK) {
        // (blockDim.x divides EMB_SUM_SCAN; EMB_SUM_SCAN slot words are loaded together, then balloted: no barrier in between, every
        //  wave writes its own mask words)
        const int per = EMB_SUM_SCAN / blockDim.x;
        for (int sub = 0; sub < EMB_SUM_CHUNK; sub += EMB_SUM_SCAN) {
            int tk[EMB_SUM_SCAN / 64];
#pragma unroll
            for (int i = 0; i < EMB_SUM_SCAN / 64; ++i) {
                const long slot = base + sub + (long)i * blockDim.x + tid;
                tk[i] = -1;
                if (i < per && slot < n_slots) tk[i] = slot_tok[slot];
            }
#pragma unroll
            for (int i = 0; i < EMB_SUM_SCAN / 64; ++i) {
                if (i >= per) break;
                const unsigned long long m = __ballot(tk[i] == v);
                if ((tid & 63) == 0) masks[(sub + i * blockDim.x + tid) >> 6] = m;
            }
        }
        __syncthreads();
        int wd = 0;
        unsigned long long mm = masks[0];          // (the same words in every thread: the loops below are uniform)
        for (bool more = true; more;) {
            f32x4 r[EMB_SUM_BATCH];
            int n = 0;
#pragma unroll
            for (int i = 0; i < EMB_SUM_BATCH; ++i) {
                while (!mm && wd + 1 < EMB_SUM_CHUNK / 64) mm = masks[++wd];
                if (!mm) break;
                const int bit = __builtin_ctzll(mm);
                mm &= mm - 1;
                if (own) r[i] = partial[(base + wd * 64 + bit) * hv + col];
                n = i + 1;
            }
#pragma unroll
            for (int i = 0; i < EMB_SUM_BATCH; ++i)
                if (i < n && own) acc += r[i];
            any |= n > 0;
            more = n == EMB_SUM_BATCH;
        }
        __syncthreads();
    }
    if (any && own) dw[(long)v * hv + col] += acc;
}

// ----------------------------------------------------------------------------------------------------------------- xent
// One row of C logits per wavefront (C <= 1024) or per 256-thread workgroup (C <= 4096); lane l holds the values c = l, l + TPR,
// ... in NV registers, so a row is read once, completely, before anything of it is written (dlogits may alias logits) and each
// gradient is written once.  The regime is HBM traffic, 2 * T * B * C * 4 bytes, plus launch latency.
constexpr int XE_THREADS = 256;
constexpr int XE_C_MAX = 4096;
constexpr int XE_LOSS_THREADS = 256;
constexpr int XE_LOSS_ROWS = 64;           // rows of the batch per workgroup of the loss kernel
constexpr int XE_LOSS_CHUNK = 128;         // time steps staged through LDS at a time (32 KiB)

typedef amdspeech_xent_plan_info XentPlan;

static int plan_xent(int T, int B, int C, XentPlan* p) {
    AS_CHECK_ARG(T > 0 && B > 0, "xent: bad shape (T %d, B %d)", T, B);
    AS_CHECK_ARG(C >= 2 && C <= XE_C_MAX, "xent: C = %d outside 2 .. %d", C, XE_C_MAX);
    AS_CHECK_ARG((long)T * B * C < (1L << 40), "xent: T * B * C too large");
    const long rows = (long)T * B;
    p->kernel = C <= 1024 ? AMDSPEECH_XENT_KERNEL_WAVE : AMDSPEECH_XENT_KERNEL_BLOCK;
    const int tpr = p->kernel == AMDSPEECH_XENT_KERNEL_WAVE ? 64 : XE_THREADS;
    const int lo = p->kernel == AMDSPEECH_XENT_KERNEL_WAVE ? 2 : 8;
    int nv = lo;
    while (nv * tpr < C) nv *= 2;
    p->values_per_lane = nv;
    p->threads = XE_THREADS;
    p->rows_per_workgroup = XE_THREADS / tpr;
    const long grid = (rows + p->rows_per_workgroup - 1) / p->rows_per_workgroup;
    AS_CHECK_ARG(grid <= 0x7fffffffL, "xent: too many rows (%ld)", rows);
    p->grid = (int)grid;
    p->c_max = nv * tpr;                                       // the range of C that takes this very kernel
    p->c_min = nv == lo ? (tpr == 64 ? 2 : 1025) : nv * tpr / 2 + 1;
    p->loss_threads = XE_LOSS_THREADS;
    p->loss_grid = ceil_div(B, XE_LOSS_ROWS);
    return AMDSPEECH_OK;
}

template <int TPR>
__device__ __forceinline__ float xe_reduce(float v, bool is_max, float* lds) {
    for (int o = 32; o > 0; o >>= 1) {
        const float u = __shfl_xor(v, o, 64);
        v = is_max ? fmaxf(v, u) : v + u;
    }
    if (TPR > 64) {                                // one row per workgroup: the four waves' values through LDS, the same order in every thread
        const int wave = threadIdx.x >> 6;
        __syncthreads();                           // (the previous reduction's reads are over)
        if ((threadIdx.x & 63) == 0) lds[wave] = v;
        __syncthreads();
        v = lds[0];
        for (int k = 1; k < TPR / 64; ++k) v = is_max ? fmaxf(v, lds[k]) : v + lds[k];
    }
    return v;
}

template <int NV, int TPR>
__global__ __launch_bounds__(XE_THREADS) void xent_rows_kernel(const float* __restrict__ logits, const int* __restrict__ targets, int ld,
                                                               const int* __restrict__ lengths, long rows, int B, int C, float scale,
                                                               float* __restrict__ nll, float* dlogits) {
    __shared__ float red[XE_THREADS / 64];
    constexpr int RPW = XE_THREADS / TPR;
    const int sub = threadIdx.x / TPR, lane = threadIdx.x - sub * TPR;
    const long row = (long)blockIdx.x * RPW + sub;
    if (row >= rows) return;                       // (a whole wave at TPR 64; never at TPR 256: one row per workgroup)
    const int t = (int)(row / B), b = (int)(row - (long)t * B);
    const int tgt = targets[(long)b * ld + t];
    const bool live = t < lengths[b] && tgt >= 0 && tgt < C;      // uniform over the row's lanes
    const float* x_row = logits + row * C;
    float* d_row = dlogits ? dlogits + row * C : nullptr;
    if (!live) {
        if (lane == 0) nll[row] = 0.0f;
        if (d_row)
            for (int i = 0; i < NV; ++i) {
                const int c = lane + i * TPR;
                if (c < C) d_row[c] = 0.0f;
            }
        return;
    }
    float x[NV];
    float m = -INFINITY, xt = 0.0f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int c = lane + i * TPR;
        x[i] = c < C ? x_row[c] : -INFINITY;
        m = fmaxf(m, x[i]);
        if (c == tgt) xt = x[i];
    }
    m = xe_reduce<TPR>(m, true, red);
    float s = 0.0f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int c = lane + i * TPR;
        x[i] = c < C ? expf(x[i] - m) : 0.0f;
        s += x[i];
    }
    s = xe_reduce<TPR>(s, false, red);
    xt = xe_reduce<TPR>(xt, false, red);           // (one lane holds the target's logit, the others 0: the sum is that value)
    if (lane == 0) nll[row] = (m + logf(s)) - xt;
    if (d_row) {
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int c = lane + i * TPR;
            if (c < C) d_row[c] = scale * (x[i] / s - (c == tgt ? 1.0f : 0.0f));
        }
    }
}

// loss[b] = the float32 rounding of the float64 sum, in increasing t, of the float32 nll[t][b]
// One workgroup per 64 rows of the batch: its four waves stage XE_LOSS_CHUNK time steps of nll through LDS (independent, coalesced
// loads), then the first wave adds them in increasing t, one row per lane.
__global__ __launch_bounds__(XE_LOSS_THREADS) void xent_loss_kernel(const float* __restrict__ nll, int T, int B, float* __restrict__ loss) {
    __shared__ float tile[XE_LOSS_CHUNK][XE_LOSS_ROWS];
    const int lane = threadIdx.x % XE_LOSS_ROWS, part = threadIdx.x / XE_LOSS_ROWS;
    const int b = blockIdx.x * XE_LOSS_ROWS + lane;
    double acc = 0.0;
    for (int t0 = 0; t0 < T; t0 += XE_LOSS_CHUNK) {
        const int n = T - t0 < XE_LOSS_CHUNK ? T - t0 : XE_LOSS_CHUNK;
        for (int i = part; i < n; i += XE_LOSS_THREADS / XE_LOSS_ROWS)
            tile[i][lane] = b < B ? nll[(long)(t0 + i) * B + b] : 0.0f;
        __syncthreads();
        if (part == 0)
            for (int i = 0; i < n; ++i) acc += (double)tile[i][lane];
        __syncthreads();
    }
    if (part == 0 && b < B) loss[b] = (float)acc;
}

template <int NV, int TPR>
static void launch_xent(hipStream_t s, const XentPlan& p, const float* logits, const int* targets, int ld, const int* lengths, long rows,
                        int B, int C, float scale, float* nll, float* dlogits) {
    hipLaunchKernelGGL((xent_rows_kernel<NV, TPR>), dim3(p.grid), dim3(p.threads), 0, s, logits, targets, ld, lengths, rows, B, C, scale,
                       nll, dlogits);
}

static bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace amdspeech

using namespace amdspeech;

static int check_tokens(const char* what, const int* ids, int ld, const int* lengths, int T, int B) {
    AS_CHECK_ARG(ids && lengths, "%s: null token or length pointer", what);
    AS_CHECK_ARG(T > 0 && B > 0, "%s: bad shape (T %d, B %d)", what, T, B);
    AS_CHECK_ARG(ld >= T, "%s: ld = %d is below T = %d", what, ld, T);
    AS_CHECK_ARG((long)B * ld < (1L << 31), "%s: B * ld too large", what);
    return AMDSPEECH_OK;
}

static int check_embed_shape(const char* what, int T, int B, int V, int H) {
    AS_CHECK_ARG(V >= 1, "%s: V = %d must be positive", what, V);
    AS_CHECK_ARG(H >= 4 && H % 4 == 0, "%s: H = %d must be a positive multiple of 4", what, H);
    AS_CHECK_ARG((long)T * B * H < (1L << 40) && (long)V * H < (1L << 40), "%s: shape too large", what);
    return AMDSPEECH_OK;
}

extern "C" int amdspeech_embed_fwd(void* stream, const int* ids, int ld, const int* lengths, int T, int B, int V, int H, const float* w,
                                   const float* bias, float* out) {
    if (int rc = check_tokens("embed_fwd", ids, ld, lengths, T, B)) return rc;
    if (int rc = check_embed_shape("embed_fwd", T, B, V, H)) return rc;
    AS_CHECK_ARG(w && out, "embed_fwd: null pointer");
    AS_CHECK_ARG(aligned16(w) && aligned16(out) && aligned16(bias), "embed_fwd: w, bias and out must be 16-byte aligned");
    const int hv = H / 4;
    const long n_words = (long)T * B * hv;
    const long wgs = (n_words + EMB_THREADS - 1) / EMB_THREADS;
    hipLaunchKernelGGL(embed_fwd_kernel, dim3((unsigned)(wgs < EMB_MAX_WGS ? wgs : EMB_MAX_WGS)), dim3(EMB_THREADS), 0,
                       static_cast<hipStream_t>(stream), ids, ld, lengths, B, V, hv, n_words, reinterpret_cast<const f32x4*>(w),
                       reinterpret_cast<const f32x4*>(bias), reinterpret_cast<f32x4*>(out));
    AS_CHECK_LAUNCH();
    return AMDSPEECH_OK;
}

extern "C" size_t amdspeech_embed_bwd_workspace_bytes(int T, int B, int V, int H) {
    if (T <= 0 || B <= 0 || check_embed_shape("embed_bwd_workspace_bytes", T, B, V, H)) return 0;
    return emb_bwd_layout(T, B, H).total;
}

extern "C" int amdspeech_embed_bwd(void* stream, const int* ids, int ld, const int* lengths, int T, int B, int V, int H, const float* dz,
                                   float* dw, float* dbias, void* ws) {
    if (int rc = check_tokens("embed_bwd", ids, ld, lengths, T, B)) return rc;
    if (int rc = check_embed_shape("embed_bwd", T, B, V, H)) return rc;
    AS_CHECK_ARG(dz && dw && ws, "embed_bwd: null pointer");
    AS_CHECK_ARG(aligned16(dz) && aligned16(dw) && aligned16(dbias) && aligned16(ws), "embed_bwd: dz, dw, dbias and ws must be 16-byte aligned");
    AS_CHECK_ARG(V < 0x7fffffff / 2, "embed_bwd: V = %d too large", V);
    const EmbBwdLayout l = emb_bwd_layout(T, B, H);
    const int hv = H / 4, threads = emb_threads(hv), col_blocks = ceil_div(hv, threads);
    AS_CHECK_ARG(col_blocks <= 65535, "embed_bwd: H = %d too large", H);
    char* base = static_cast<char*>(ws);
    int* slot_tok = reinterpret_cast<int*>(base + l.slot_tok);
    int* seg_live = reinterpret_cast<int*>(base + l.seg_live);
    f32x4* bias_part = reinterpret_cast<f32x4*>(base + l.bias_part);
    f32x4* partial = reinterpret_cast<f32x4*>(base + l.partial);
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(embed_bwd_partial_kernel, dim3(l.n_seg, col_blocks), dim3(threads), 0, s, ids, ld, lengths, (long)T * B, B, V, hv,
                       reinterpret_cast<const f32x4*>(dz), slot_tok, seg_live, dbias ? bias_part : nullptr, partial);
    AS_CHECK_LAUNCH();
    hipLaunchKernelGGL(embed_bwd_sum_kernel, dim3(V + 1, col_blocks), dim3(threads), 0, s, V, hv, l.n_seg, l.n_slots, slot_tok, seg_live,
                       bias_part, partial, reinterpret_cast<f32x4*>(dw), reinterpret_cast<f32x4*>(dbias));
    AS_CHECK_LAUNCH();
    return AMDSPEECH_OK;
}

extern "C" int amdspeech_xent_plan(int T, int B, int C, amdspeech_xent_plan_info* out) {
    AS_CHECK_ARG(out != nullptr, "xent_plan: null output");
    return plan_xent(T, B, C, out);
}

extern "C" size_t amdspeech_xent_workspace_bytes(int T, int B, int C) {
    XentPlan p;
    if (plan_xent(T, B, C, &p)) return 0;
    return align_up((size_t)T * B * 4, 256);       // nll when the caller does not want it
}

extern "C" int amdspeech_xent_fwd_bwd(void* stream, const float* logits, const int* targets, int ld, const int* lengths, int T, int B, int C,
                                      float scale, float* nll, float* loss, float* dlogits, void* ws) {
    XentPlan p;
    if (int rc = plan_xent(T, B, C, &p)) return rc;
    if (int rc = check_tokens("xent_fwd_bwd", targets, ld, lengths, T, B)) return rc;
    AS_CHECK_ARG(logits && loss && ws, "xent_fwd_bwd: null pointer");
    AS_CHECK_ARG((reinterpret_cast<uintptr_t>(ws) & 3) == 0, "xent_fwd_bwd: ws must be 4-byte aligned");
    if (dlogits && dlogits != logits) {
        const uintptr_t a = reinterpret_cast<uintptr_t>(logits), d = reinterpret_cast<uintptr_t>(dlogits), n = (uintptr_t)T * B * C * 4;
        AS_CHECK_ARG(a + n <= d || d + n <= a, "xent_fwd_bwd: dlogits overlaps logits without being the same buffer");
    }
    float* nll_buf = nll ? nll : static_cast<float*>(ws);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const long rows = (long)T * B;
    const bool wave = p.kernel == AMDSPEECH_XENT_KERNEL_WAVE;
#define XE_CASE(NV, TPR) launch_xent<NV, TPR>(s, p, logits, targets, ld, lengths, rows, B, C, scale, nll_buf, dlogits)
    switch (p.values_per_lane) {
        case 2: XE_CASE(2, 64); break;
        case 4: XE_CASE(4, 64); break;
        case 8: if (wave) XE_CASE(8, 64); else XE_CASE(8, 256); break;
        case 16: if (wave) XE_CASE(16, 64); else XE_CASE(16, 256); break;
        default: AS_CHECK_ARG(false, "xent_fwd_bwd: no kernel for %d values per lane", p.values_per_lane);
    }
#undef XE_CASE
    AS_CHECK_LAUNCH();
    hipLaunchKernelGGL(xent_loss_kernel, dim3(p.loss_grid), dim3(p.loss_threads), 0, s, nll_buf, T, B, loss);
    AS_CHECK_LAUNCH();
    return AMDSPEECH_OK;
}
