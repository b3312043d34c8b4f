// CTC forced alignment (Viterbi): the best alignment of a known transcript to the frames.  Included by ctc.hip after its kernels:
// the extended targets (ctc_prepare_kernel), the log-softmax (log_softmax_kernel) and the argument checks (ctc_check_shape) are
// the loss's own, so the aligner keeps and ignores exactly the rows the loss keeps and ignores.
//
// Two kernels.  ctc_viterbi_kernel runs the alpha recursion with the log-sum-exp replaced by a maximum and leaves a 2-bit
// back-pointer per (frame, state); ctc_backtrace_kernel walks the pointers from the last frame to the first and forms the outputs.
// Neither waits on another workgroup.
//
// Ties are part of the contract (amdspeech.h): the SMALLEST step wins -- stay, then s-1, then s-2 -- and at the last frame state
// S-1 wins over S-2.
#pragma once
#include "common.h"
#include "ctc_core.h"

namespace amdspeech {

struct CtcAlignLayout { size_t logp, ext, slen, valid, fin, vscore, bp, total; int smax, pitch; };  // byte offsets

// bp: [B][T][pitch] bytes, byte j of a row holds the pointers of states 4j .. 4j+3 (2 bits each, state 4j lowest); the pitch is
// rounded up to whole dwords so that the backtrace stages rows with aligned 4-byte loads
static CtcAlignLayout ctc_align_layout(int T, int B, int C, int U) {
    CtcAlignLayout o;
    o.smax = 2 * U + 1;
    o.pitch = (int)align_up((size_t)(o.smax + 3) / 4, 4);
    size_t off = 0;
    auto take = [&](size_t bytes) { size_t r = off; off += align_up(bytes, 256); return r; };
    o.logp = take((size_t)T * B * C * 4);
    o.ext = take((size_t)B * o.smax * 4);
    o.slen = take((size_t)B * 4);
    o.valid = take((size_t)B * 4);
    o.fin = take((size_t)B * 4);
    o.vscore = take((size_t)B * 4);
    o.bp = take((size_t)B * T * o.pitch);
    o.total = off;
    return o;
}

// ---- the recursion: one workgroup of NW waves per utterance, thread i owns the RMAX adjacent states i*RMAX .. i*RMAX+RMAX-1 ----
// RMAX is the layout itself here (not an upper bound as in ctc_alpha_beta_kernel): with RMAX a multiple of 4 a thread owns whole
// bytes of the back-pointer row and stores them alone; with RMAX = 2 two neighbouring lanes join their nibbles by one DPP move.
// A step needs the previous frame's states s-1 and s-2: in-thread but for the thread's first two states, which take the last two
// of thread i-1 -- by a DPP wave shift in the one-wave layout (NW = 1, no LDS, no barrier), through the parity-double-buffered LDS
// edge array with one barrier per frame in the four-wave layout.  The state is float64 over the float32 log-softmax emissions
// (natural logs; nothing is rescaled: there is no transcendental in the loop): a float32 state rounds at the magnitude of the
// running score at every frame and ends 2e-2 nats off at T ~ 2400, which is more than the margin between neighbouring paths.
// The emission gathers are prefetched a block of PF frames ahead, as in the alpha / beta kernels.
template <int RMAX, int PF, int NW>
__global__ __launch_bounds__(NW * 64) void ctc_viterbi_kernel(const float* __restrict__ logp, const int* __restrict__ ext,
                                                              const int* __restrict__ slen, const int* __restrict__ valid,
                                                              const int* __restrict__ lengths, int T, int B, int C, int smax,
                                                              int pitch, unsigned char* __restrict__ bp, int* __restrict__ fin,
                                                              float* __restrict__ vscore) {
    static_assert(RMAX == 2 || RMAX % 4 == 0, "a thread owns a nibble (with its neighbour: a byte) or whole bytes of a back-pointer row");
    static_assert(NW == 4 || (NW == 1 && RMAX == 2), "one wave of two states per lane, or four waves");
    constexpr int NT = NW * 64, NB = (RMAX + 3) / 4;
    __shared__ double2 edge[2][NT + 1];      // [parity][1 + thread]: a pad of -inf in front
    __shared__ double last2[2];              // the last frame's states S-1, S-2
    constexpr double NEG_INF_D = -__builtin_inf();
    const int b = blockIdx.x, tid = threadIdx.x;
    if (!valid[b]) { if (tid == 0) { vscore[b] = 0.f; fin[b] = -1; } return; }
    const int S = slen[b];
    const int Tb = min(lengths[b], T);
    const int blank = C - 1;
    const int* e = ext + (size_t)b * smax;
    int lab[RMAX]; bool skip[RMAX]; bool act[RMAX];
#pragma unroll
    for (int r = 0; r < RMAX; ++r) {
        const int s = tid * RMAX + r;
        act[r] = s < S;
        lab[r] = act[r] ? e[s] : blank;
        skip[r] = act[r] && s >= 2 && lab[r] != blank && lab[r] != e[s - 2];
    }
    if (tid == 0) {
        if constexpr (NW > 1) {
            edge[0][0] = make_double2(NEG_INF_D, NEG_INF_D);
            edge[1][0] = make_double2(NEG_INF_D, NEG_INF_D);
        }
        last2[0] = NEG_INF_D; last2[1] = NEG_INF_D;
    }
    const size_t rowstride = (size_t)B * C;
    const float* lp = logp + (size_t)b * C;
    unsigned char* rows = bp + (size_t)b * T * pitch;

    double cur[RMAX];
#pragma unroll
    for (int r = 0; r < RMAX; ++r) cur[r] = (act[r] && tid * RMAX + r < 2) ? (double)lp[lab[r]] : NEG_INF_D;

    auto load_block = [&](int i0, float (&buf)[PF][RMAX]) {
#pragma unroll
        for (int q = 0; q < PF; ++q) {
            const int i = min(i0 + q, Tb - 1);                  // clamped: loads stay unconditional
#pragma unroll
            for (int r = 0; r < RMAX; ++r) buf[q][r] = lp[(size_t)i * rowstride + lab[r]];
        }
    };
    auto step = [&](int i, const float (&lpv)[RMAX]) {
        double p1, p2;                                          // the previous frame's states s-1, s-2 of this thread's first state
        if constexpr (NW == 1) {
            p1 = ctc_from_lane_below(cur[RMAX - 1]);
            p2 = ctc_from_lane_below(cur[RMAX - 2]);
        } else {
            double2* ed = edge[i & 1] + 1;                      // ed[thread]
            ed[tid] = make_double2(cur[RMAX - 1], cur[RMAX - 2]);
            ctc_frame_barrier();
            const double2 n1 = ed[tid - 1];
            p1 = n1.x; p2 = n1.y;
        }
        unsigned bits[NB];
#pragma unroll
        for (int j = 0; j < NB; ++j) bits[j] = 0u;
#pragma unroll
        for (int r = 0; r < RMAX; ++r) {
            const double a = cur[r], c2 = skip[r] ? p2 : NEG_INF_D;
            // the smallest step wins a tie: stay, then s-1, then s-2 (all three at -inf: "stay", never followed)
            const bool stay = a >= p1 && a >= c2, one = p1 >= c2;
            const double m = stay ? a : one ? p1 : c2;
            const unsigned k = stay ? 0u : one ? 1u : 2u;
            bits[r / 4] |= k << ((r % 4) * 2);
            cur[r] = m + (double)lpv[r];                        // (states >= S run along on the blank's emission: nothing below S reads them)
            p2 = p1; p1 = a;
        }
        unsigned char* row = rows + (size_t)i * pitch;
        if constexpr (RMAX == 2) {
            // states 4j, 4j+1 sit in lane 2j, states 4j+2, 4j+3 in lane 2j+1: the even lane stores the byte
            const unsigned other = (unsigned)__builtin_amdgcn_update_dpp(0, (int)bits[0], 0xB1 /* quad_perm:[1,0,3,2] */, 0xf, 0xf, false);
            if ((tid & 1) == 0 && tid * 2 < S) row[tid >> 1] = (unsigned char)(bits[0] | (other << 4));
        } else if constexpr (RMAX == 8) {
            if (tid * 8 < S) *reinterpret_cast<unsigned short*>(row + tid * 2) = (unsigned short)(bits[0] | (bits[1] << 8));
        } else if constexpr (RMAX == 16) {
            if (tid * 16 < S) *reinterpret_cast<unsigned*>(row + tid * 4) = bits[0] | (bits[1] << 8) | (bits[2] << 16) | (bits[3] << 24);
        } else {
#pragma unroll
            for (int j = 0; j < NB; ++j) if (tid * RMAX + 4 * j < S) row[tid * NB + j] = (unsigned char)bits[j];
        }
    };

    if (Tb > 1) {
        float bufA[PF][RMAX], bufB[PF][RMAX];
        load_block(1, bufA);
        for (int i0 = 1; i0 < Tb; i0 += 2 * PF) {
            load_block(i0 + PF, bufB);
#pragma unroll
            for (int q = 0; q < PF; ++q) if (i0 + q < Tb) step(i0 + q, bufA[q]);
            load_block(i0 + 2 * PF, bufA);
#pragma unroll
            for (int q = 0; q < PF; ++q) if (i0 + PF + q < Tb) step(i0 + PF + q, bufB[q]);
        }
    }
    // the best path ends in S-1 or S-2; S-1 wins a tie
    __syncthreads();
#pragma unroll
    for (int r = 0; r < RMAX; ++r) {
        const int s = tid * RMAX + r;
        if (act[r] && s == S - 1) last2[0] = cur[r];
        if (act[r] && s == S - 2) last2[1] = cur[r];
    }
    __syncthreads();
    if (tid == 0) {
        const double a = last2[0], c = last2[1];
        const double m = a >= c ? a : c;
        vscore[b] = (float)m;
        fin[b] = m == NEG_INF_D ? -1 : (a >= c ? S - 1 : S - 2);      // -1: no alignment exists (the loss is inf on such a row)
    }
}

// ---- the walk back: one wave per utterance ---------------------------------------------------------------------------
// The walk is serial in t and a dependent global load per frame would cost T memory latencies, so the pointers of a block of BT_F
// frames are staged in LDS by the whole wave and lane 0 walks the block there.  A path drops by at most two states per frame, so
// of each row only the BT_W bytes below the state the block is entered in can be reached: that window is all that is staged
// (2.5 KiB a block, whatever the width of the target).  Lane 0 leaves the block's states in LDS; then the wave forms the block's
// outputs in parallel, lane i for frame t0 + i: label, state, the first / last frame of a label, and the sum of log p over the
// label's frames (the lane of a label's first frame in the block adds up the run; a path is monotone, so a label has ONE run per
// block and nobody else touches its accumulator).  Per-label accumulators live in LDS: 16 bytes a label.
constexpr int BT_F = 64, BT_W = 40;      // frames per block; bytes of a row staged: 2 * 64 states = 32 bytes + the byte of the entry state + dword alignment
__global__ __launch_bounds__(64) void ctc_backtrace_kernel(const float* __restrict__ logp, const int* __restrict__ ext,
                                                           const int* __restrict__ slen, const int* __restrict__ lengths,
                                                           const unsigned char* __restrict__ bp, const int* __restrict__ fin,
                                                           const float* __restrict__ vscore, int T, int B, int C, int U, int smax,
                                                           int pitch, int* __restrict__ frame_label, int* __restrict__ frame_state,
                                                           int* __restrict__ spans, float* __restrict__ score,
                                                           float* __restrict__ confidence) {
    extern __shared__ double lsum[];                     // [U] sum of log p over the label's frames, then int first[U], last[U]
    __shared__ unsigned win[BT_F][BT_W / 4];
    __shared__ int st[BT_F + 2];                         // st[1 + i]: state at frame t0 + i; st[0], st[n + 1]: the frames beside the block (-1: none)
    __shared__ float lpv[BT_F];
    int* first = reinterpret_cast<int*>(lsum + U);
    int* last = first + U;
    const int b = blockIdx.x, lane = threadIdx.x;
    const int fs = fin[b];
    const int Tb = fs >= 0 ? min(lengths[b], T) : 0;     // ignored rows and rows without an alignment: -1 everywhere
    int* fl = frame_label + (size_t)b * T;
    int* fst = frame_state + (size_t)b * T;
    for (int t = Tb + lane; t < T; t += 64) { fl[t] = -1; fst[t] = -1; }
    for (int u = lane; u < U; u += 64) { lsum[u] = 0.0; first[u] = -1; last[u] = -1; }
    if (lane == 0) score[b] = vscore[b];
    const int* e = ext + (size_t)b * smax;
    const unsigned char* rows = bp + (size_t)b * T * pitch;
    const size_t rowstride = (size_t)B * C;
    const float* lp = logp + (size_t)b * C;
    int s = fs, above = -1;                              // the state the block is entered in (at t1); the state at t1 + 1
    for (int t1 = Tb - 1; t1 >= 0; t1 -= BT_F) {
        const int t0 = max(t1 - (BT_F - 1), 0), n = t1 - t0 + 1;
        const int lo = s >= 4 * (BT_W - 8) ? ((s >> 2) - (BT_W - 8)) & ~3 : 0;      // first byte of the window (s/4 <= lo + BT_W - 5)
        for (int idx = lane; idx < n * (BT_W / 4); idx += 64) {
            const int f = idx / (BT_W / 4), dw = idx % (BT_W / 4);
            const int t = t1 - f, off = lo + dw * 4;
            win[f][dw] = (t >= 1 && off < pitch) ? *reinterpret_cast<const unsigned*>(rows + (size_t)t * pitch + off) : 0u;
        }
        __syncthreads();
        if (lane == 0) {
            int cs = s;
            for (int f = 0; f < n; ++f) {
                st[n - f] = cs;
                const int rel = cs - 4 * lo;             // 0 <= rel < 4 * BT_W: cs >= s - 2 f > 4 lo
                if (t1 - f >= 1) cs -= (int)((win[f][rel >> 4] >> ((rel & 15) * 2)) & 3u);
            }
            st[0] = t0 > 0 ? cs : -1;
            st[n + 1] = above;
        }
        __syncthreads();
        const bool on = lane < n;
        const int my = on ? st[lane + 1] : -1, prev = on ? st[lane] : -1, next = on ? st[lane + 2] : -1;
        const int t = t0 + lane;
        if (on) {
            const int l = e[my];
            lpv[lane] = lp[(size_t)t * rowstride + l];
            fl[t] = l; fst[t] = my;
        }
        __syncthreads();
        if (on && (my & 1)) {
            const int u = my >> 1;
            if (prev != my) first[u] = t;
            if (next != my) last[u] = t;
            if (prev != my || lane == 0) {
                double acc = 0.0;
                for (int j = lane; j < n && st[j + 1] == my; ++j) acc += (double)lpv[j];
                lsum[u] += acc;
            }
        }
        above = st[1];
        s = st[0];
        __syncthreads();
    }
    __syncthreads();
    for (int u = lane; u < U; u += 64) {
        const int f0 = first[u], f1 = last[u];
        spans[((size_t)b * U + u) * 2] = f0;
        spans[((size_t)b * U + u) * 2 + 1] = f1;
        confidence[(size_t)b * U + u] = f0 >= 0 ? (float)exp(lsum[u] / (double)(f1 - f0 + 1)) : 0.f;
    }
}

// ---- which instantiation a shape takes: the ONE place that decides (amdspeech_ctc_align and amdspeech_ctc_align_plan read it) ----
static int ctc_align_plan(int T, int B, int C, int U, CtcPlan* p) {
    if (int rc = ctc_check_shape(T, B, C, U)) return rc;
    const int smax = 2 * U + 1;
    if (smax <= 128) { *p = CtcPlan{AMDSPEECH_CTC_KERNEL_WAVE, 64, 2, smax}; return AMDSPEECH_OK; }
    const int rneed = ceil_div(smax, 256);
    *p = CtcPlan{AMDSPEECH_CTC_KERNEL_EDGE, 256, rneed <= 2 ? 2 : rneed <= 4 ? 4 : rneed <= 8 ? 8 : rneed <= 12 ? 12 : rneed <= 16 ? 16 : 20, smax};
    return AMDSPEECH_OK;
}

}  // namespace amdspeech

extern "C" size_t amdspeech_ctc_align_workspace_bytes(int T, int B, int C, int U) {
    if (T <= 0 || B <= 0 || C <= 1 || U <= 0) return 0;
    return amdspeech::ctc_align_layout(T, B, C, U).total;
}

extern "C" int amdspeech_ctc_align_plan(int T, int B, int C, int U, amdspeech_ctc_plan_info* out) {
    using namespace amdspeech;
    AS_CHECK_ARG(out != nullptr, "ctc_align_plan: null output");
    CtcPlan p;
    if (int rc = ctc_align_plan(T, B, C, U, &p)) return rc;
    *out = amdspeech_ctc_plan_info{p.kernel, p.threads, p.rmax, p.smax};
    return AMDSPEECH_OK;
}

extern "C" int amdspeech_ctc_align(void* stream, const float* logits, const int* dense_labels, const int* lengths, int T, int B,
                                   int C, int U, int* frame_label, int* frame_state, int* spans, float* score, float* confidence,
                                   void* ws) {
    using namespace amdspeech;
    CtcPlan plan;
    if (int rc = ctc_align_plan(T, B, C, U, &plan)) return rc;
    AS_CHECK_ARG(logits && dense_labels && lengths && frame_label && frame_state && spans && score && confidence && ws,
                 "ctc_align: null pointer");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const CtcAlignLayout lo = ctc_align_layout(T, B, C, U);
    char* w = static_cast<char*>(ws);
    float* logp = reinterpret_cast<float*>(w + lo.logp);
    int* ext = reinterpret_cast<int*>(w + lo.ext);
    int* slen = reinterpret_cast<int*>(w + lo.slen);
    int* valid = reinterpret_cast<int*>(w + lo.valid);
    int* fin = reinterpret_cast<int*>(w + lo.fin);
    float* vscore = reinterpret_cast<float*>(w + lo.vscore);
    unsigned char* bp = reinterpret_cast<unsigned char*>(w + lo.bp);
    const long rows = (long)T * B;
    hipLaunchKernelGGL(ctc_prepare_kernel, dim3(B), dim3(64), 0, s, dense_labels, lengths, T, U, C, lo.smax, ext, slen, valid);
    hipLaunchKernelGGL(log_softmax_kernel, dim3(ceil_div(rows, 4)), dim3(256), 0, s, logits, logp, rows, C);
#define LAUNCH_V(R, PF, NW) hipLaunchKernelGGL((ctc_viterbi_kernel<R, PF, NW>), dim3(B), dim3(NW * 64), 0, s, logp, ext, slen, valid, lengths, T, B, C, lo.smax, lo.pitch, bp, fin, vscore)
    if (plan.kernel == AMDSPEECH_CTC_KERNEL_WAVE) LAUNCH_V(2, 8, 1);
    else if (plan.rmax == 2) LAUNCH_V(2, 8, 4);
    else if (plan.rmax == 4) LAUNCH_V(4, 8, 4);
    else if (plan.rmax == 8) LAUNCH_V(8, 4, 4);
    else if (plan.rmax == 12) LAUNCH_V(12, 4, 4);
    else if (plan.rmax == 16) LAUNCH_V(16, 4, 4);
    else LAUNCH_V(20, 4, 4);
#undef LAUNCH_V
    hipLaunchKernelGGL(ctc_backtrace_kernel, dim3(B), dim3(64), (size_t)U * 16, s, logp, ext, slen, lengths, bp, fin, vscore, T, B, C, U,
                       lo.smax, lo.pitch, frame_label, frame_state, spans, score, confidence);
    AS_CHECK_LAUNCH();
    return AMDSPEECH_OK;
}
