// Stacked-LSTM forward and BPTT for gfx950 (replaces BasicLSTMCell + DropoutWrapper +
// MultiRNNCell + dynamic_rnn, /root/reference/models/AcousticModel.py:223-237,266-298).
//
// Design (MI355X-first):
//  * The recurrence is latency bound: per frame and layer the dependent product is
//    only [B, 2H] x [2H, 4H].  All L layers advance together along the anti-diagonal
//    d = t + l (wavefront pipelining), so the dependent chain is T+L-1 short kernels,
//    not T*L; each launch is cut at the h all-gather seam (a kernel boundary costs
//    ~1.5 us on this chip, less than any in-kernel grid barrier).
//  * A workgroup owns a slice of hidden units for ALL four gates, so the gate
//    non-linearities, the cell update, length masking and dropout are fused behind
//    the MFMAs and nothing but h/c/gates ever goes back to HBM.
//  * [x_t ; h_{t-1}] . K uses v_mfma_f32_16x16x4_f32 (exact f32).  The 2H-long K axis
//    is split across the 4 waves of a workgroup (one per SIMD), reduced through LDS.
//  * Weights are repacked once per optimiser step into MFMA B-fragment order: one
//    fully coalesced 1 KiB float4 load per wave feeds four MFMAs; the slices stay
//    L2/MALL resident across the T launches (24 MB total for 3x512).
//  * BPTT runs the mirrored diagonal: dh_t = dG_{t+1} . W_hh^T (+ dG^{l+1}_t . W_ih^T
//    from the layer above) fused with the gate-gradient math; the weight gradients
//    dK = [Z ; Hprev]^T . dG are time-independent and go to the big split-K GEMM.
#include "common.h"
#include "gemm_core.h"
#include "ctc_core.h"
#include <stdlib.h>
#include <string.h>
#include <type_traits>
#include <mutex>
#include <unordered_map>

namespace amdspeech {

// s_waitcnt vmcnt(0) (expcnt / lgkmcnt untouched) in a form the compiler's own wait-count bookkeeping sees.  The whole-sequence
// kernels load their weight fragments once, in front of the time loop; without this in front of the loop hipcc merges "weight
// loads still pending" into the loop header and guards the first use of every weight register INSIDE the loop with a ladder of
// s_waitcnt vmcnt(n) ... vmcnt(0) in the middle of the MFMA stream, which at run time waits for whatever the wave has in flight
// then (in lstm_bwd_big: the write-through store of the row-major dG tile it has just issued).
#define FLOW_WEIGHTS_RESIDENT() __builtin_amdgcn_s_waitcnt(0x0F70)
// In-kernel wall-clock stamps / debug taps (tools/trace_*.py) write through a device pointer the TOOL hands over in
// AMDSPEECH_TRACE_PTR: development builds (-DAMDSPEECH_DEVTRACE) only -- a release library never takes an address from the
// environment.
static unsigned long long* dev_trace_ptr() {
#ifdef AMDSPEECH_DEVTRACE
    if (const char* e = dev_knob_str("AMDSPEECH_TRACE_PTR")) return reinterpret_cast<unsigned long long*>(strtoull(e, nullptr, 0));
#endif
    return nullptr;
}
#ifndef BIG_WEIGHTS_RESIDENT
#define BIG_WEIGHTS_RESIDENT 1    // (dev: 0 = the H = 1024 kernels without it)
#endif

// ------------------------------------------------------------------ workspace
struct LstmLayout {
    size_t wp, wq, z, hs, cs, gates, dg, dztop, dz0, dc, xp0, xp, hp, dgp, sync, xph, hph, dxh, prec, pdown, xwp, bigring, wopack, bfs, total;  // float offsets
    size_t fwd_set = 0;     // distance (floats) between the two sets of forward panels {xph, hph}
};

// The dataflow ("flow") kernels keep a workgroup's weight slice on chip for the whole sequence and place one
// recurrence group (layer, 16-row batch tile) per XCD: H a multiple of 128 up to 512, at most 8 groups.
static bool flow_shape_ok(const amdspeech_lstm_desc* d) {
    // (the kernels address one layer's [T][B][4H] gradients through a 32-bit buffer resource)
    // (split precision pairs K blocks: H a multiple of 256 there)
    return (d->precision == 0 || ((d->precision == 1 || d->precision == 2) && d->H % 256 == 0)) && d->H % 128 == 0 && d->H <= 512 && (long)d->L * ((d->B + 15) / 16) <= 8 &&
           (size_t)d->T * ((d->B + 15) / 16 * 16) * 4 * d->H * 4 < (1ull << 32);
}
// x-product workers of the forward dataflow kernel (fwd_x_worker): exact f32 at H = 512, at least one XCD without a recurrence group,
// and the tile history (one K block per recurrence wave and half) addressable through one 32-bit buffer resource.  (Two K blocks per
// wave were built and measured slower: DESIGN.md 4.2.)
static bool fwd_workers_fit(const amdspeech_lstm_desc* d) {
    const long groups = (long)d->L * ((d->B + 15) / 16);
    return d->precision == 0 && d->H == 512 && groups < 8 && (size_t)d->T * groups * (d->H / 16) * 4096 < (1ull << 32);
}
// FWD2_WORKER_RESERVE workgroups of every spare XCD exit at once: their CUs are what work ordered behind
// amdspeech_lstm_beside_forward (the next mini-batch's front end, the side-stream fills) runs on.
#ifndef FWD2_WORKER_RESERVE
#define FWD2_WORKER_RESERVE 8
#endif
// worker workgroups per spare XCD when `waves` waves of each take a full role (callers: fwd_workers_fit holds)
static int fwd_worker_wgs_per_xcd(const amdspeech_lstm_desc* d, int waves) {
    const int groups = d->L * ((d->B + 15) / 16), spare = 8 - groups;
    const int wgs = (groups * (d->H / 16) + waves - 1) / waves;
    return (wgs + spare - 1) / spare;
}
// ... and the half roles (lstm_flow_fwd.h): where the full roles fit one per SIMD -- waves 0-3, so waves 4-7 are free -- and a
// frame of a tile and a half per role keeps the history inside its 32-bit buffer resource
static bool fwd_half_roles_fit(const amdspeech_lstm_desc* d) {
    const long groups = (long)d->L * ((d->B + 15) / 16);
    return fwd_workers_fit(d) && fwd_worker_wgs_per_xcd(d, 4) <= 32 - FWD2_WORKER_RESERVE &&
           (size_t)d->T * groups * (d->H / 16) * 6144 < (1ull << 32);
}
// ---- the batched products of the H = 1024 path through bf16 copies (precision = 2; gemm_bf16p.hip) ----------------------------------
// One region of the workspace: Z as bf16 [TB][H] (x . W_ih), W_ih^T [4H][H]; dG as bf16 [TB][4H] and W_ih [H][4H] (dX);
// [Z ; Hprev]^T [2H][TB] and dG^T [4H][TB] (dK, both halves of a layer's kernel gradient as ONE product); the partial tiles of dK.
// The region is RESERVED for every sequence length of the shape (ops.LstmWorkspace lays ONE allocation out for the longest sequence and
// re-lays it out per mini-batch with a shorter T: a layout's size has to be monotone in T) and USED by the calls whose row count the
// 64 x 64 transposing copies take; the others fall back to gemm_bf16 inside the same layout.
static bool bf16p_layout_reserved(const amdspeech_lstm_desc* d) {
    static const int env = runtime_switch("AMDSPEECH_BF16_PACKED", 1);      // 0: gemm_bf16 (f32 operands converted on the way into LDS: round 4)
    return env != 0 && d->precision == 2 && d->H == 1024;
}
static bool bf16p_layout_on(const amdspeech_lstm_desc* d) {
    return bf16p_layout_reserved(d) && ((long)d->T * d->B) % 64 == 0 && (long)d->T * d->B >= 256;
}
struct Bf16pBufs { unsigned short *zb, *wtb, *dgb, *wb, *zht, *dgt; char* partial; size_t partial_bytes; };
static size_t bf16p_scratch_floats(const amdspeech_lstm_desc* d) {
    const size_t TB = ((size_t)d->T * d->B + 63) / 64 * 64, H = d->H;      // (reserved for every T: see bf16p_layout_reserved)
    const size_t bytes = TB * H * 2 + 4 * H * H * 2 + TB * 4 * H * 2 + H * 4 * H * 2 + 2 * H * TB * 2 + 4 * H * TB * 2 +
                         bf16p_partial_bytes_max() + 8 * 256;
    return (bytes + 3) / 4;
}
static Bf16pBufs bf16p_bufs(const amdspeech_lstm_desc* d, float* base) {
    const size_t TB = (size_t)d->T * d->B, H = d->H;
    char* p = reinterpret_cast<char*>(base);
    auto take = [&](size_t bytes) { char* r = p; p += align_up(bytes, 256); return r; };
    Bf16pBufs b;
    b.zb = reinterpret_cast<unsigned short*>(take(TB * H * 2));
    b.wtb = reinterpret_cast<unsigned short*>(take(4 * H * H * 2));
    b.dgb = reinterpret_cast<unsigned short*>(take(TB * 4 * H * 2));
    b.wb = reinterpret_cast<unsigned short*>(take(H * 4 * H * 2));
    b.zht = reinterpret_cast<unsigned short*>(take(2 * H * TB * 2));
    b.dgt = reinterpret_cast<unsigned short*>(take(4 * H * TB * 2));
    b.partial_bytes = bf16p_partial_bytes_max();      // (whatever the row count: the region's size stays monotone in T)
    b.partial = take(b.partial_bytes);
    return b;
}
// G[rows][4H] = Z[rows][H] . K[0:H, :] + bias
static int bf16p_xw(hipStream_t s, const Bf16pBufs& b, int rows, int H, const float* Z, const float* K, float* G, const float* bias) {
    if (int rc = bf16p_copy(s, Z, H, rows, H, false, b.zb, H, nullptr)) return rc;
    if (int rc = bf16p_copy(s, K, 4 * H, H, 4 * H, true, b.wtb, H, nullptr)) return rc;              // [H][4H] -> [4H][H]
    return bf16p_gemm(s, rows, 4 * H, H, b.zb, H, b.wtb, H, G, 4 * H, bias, false, b.partial, b.partial_bytes);
}
// dX[rows][H] = dG[rows][4H] . K[0:H, :]^T
static int bf16p_dx(hipStream_t s, const Bf16pBufs& b, int rows, int H, const float* dG, const float* K, float* dX) {
    if (int rc = bf16p_copy(s, dG, 4 * H, rows, 4 * H, false, b.dgb, 4 * H, nullptr)) return rc;
    if (int rc = bf16p_copy(s, K, 4 * H, H, 4 * H, false, b.wb, 4 * H, nullptr)) return rc;
    return bf16p_gemm(s, rows, H, 4 * H, b.dgb, 4 * H, b.wb, 4 * H, dX, H, nullptr, false, b.partial, b.partial_bytes);
}
// A whole layer's batched backward products behind its recurrence launch (all T x B rows): ONE read of dG gives its row-major
// copy (dX), its transposed copy (dK) and the bias gradient; dX[rows][H] = dG . K[0:H, :]^T; dK[2H][4H] += [Z ; Hprev]^T . dG
static int bf16p_layer_bwd(hipStream_t s, const Bf16pBufs& b, int rows, int H, const float* Z, const float* Hp, const float* dG, const float* K,
                           float* dX, float* dK, float* dbias) {
    if (int rc = bf16p_copy(s, dG, 4 * H, rows, 4 * H, true, b.dgt, rows, dbias, b.dgb)) return rc;
    if (int rc = bf16p_copy(s, K, 4 * H, H, 4 * H, false, b.wb, 4 * H, nullptr)) return rc;
    if (int rc = bf16p_gemm(s, rows, H, 4 * H, b.dgb, 4 * H, b.wb, 4 * H, dX, H, nullptr, false, b.partial, b.partial_bytes)) return rc;
    if (int rc = bf16p_copy(s, Z, H, rows, H, true, b.zht, rows, nullptr)) return rc;
    if (int rc = bf16p_copy(s, Hp, H, rows, H, true, b.zht + (size_t)H * rows, rows, nullptr)) return rc;
    return bf16p_gemm(s, 2 * H, 4 * H, rows, b.zht, rows, b.dgt, rows, dK, 4 * H, nullptr, true, b.partial, b.partial_bytes);
}
// ... when the recurrence kernel has written dG's row-major bf16 copy and its column sums itself (lstm_bwd_big1)
static int bf16p_layer_bwd_copied(hipStream_t s, const Bf16pBufs& b, int rows, int H, const float* Z, const float* Hp, const float* K,
                                  float* dX, float* dK) {
    if (int rc = bf16p_copy(s, K, 4 * H, H, 4 * H, false, b.wb, 4 * H, nullptr)) return rc;
    if (int rc = bf16p_gemm(s, rows, H, 4 * H, b.dgb, 4 * H, b.wb, 4 * H, dX, H, nullptr, false, b.partial, b.partial_bytes)) return rc;
    if (int rc = bf16p_copy(s, Z, H, rows, H, true, b.zht, rows, nullptr)) return rc;
    if (int rc = bf16p_copy(s, Hp, H, rows, H, true, b.zht + (size_t)H * rows, rows, nullptr)) return rc;
    if (int rc = bf16p_transpose(s, b.dgb, rows, 4 * H, b.dgt, rows)) return rc;
    return bf16p_gemm(s, 2 * H, 4 * H, rows, b.zht, rows, b.dgt, rows, dK, 4 * H, nullptr, true, b.partial, b.partial_bytes);
}
// dK[2H][4H] += [Z ; Hprev]^T . dG over `rows` frames x batch rows (a multiple of 64); dbias[4H] += column sums of dG
static int bf16p_dk(hipStream_t s, const Bf16pBufs& b, int rows, int H, const float* Z, const float* Hp, const float* dG, float* dK, float* dbias) {
    if (int rc = bf16p_copy(s, Z, H, rows, H, true, b.zht, rows, nullptr)) return rc;
    if (int rc = bf16p_copy(s, Hp, H, rows, H, true, b.zht + (size_t)H * rows, rows, nullptr)) return rc;
    if (int rc = bf16p_copy(s, dG, 4 * H, rows, 4 * H, true, b.dgt, rows, dbias)) return rc;
    return bf16p_gemm(s, 2 * H, 4 * H, rows, b.zht, rows, b.dgt, rows, dK, 4 * H, nullptr, true, b.partial, b.partial_bytes);
}

static int check_desc(const amdspeech_lstm_desc* d) {
    AS_CHECK_ARG(d != nullptr, "lstm: null descriptor");
    AS_CHECK_ARG(d->T > 0 && d->B > 0 && d->H > 0 && d->L > 0, "lstm: bad shape T=%d B=%d H=%d L=%d",
                 d->T, d->B, d->H, d->L);
    AS_CHECK_ARG(d->H % 16 == 0, "lstm: hidden size %d must be a multiple of 16", d->H);
    AS_CHECK_ARG(d->keep_in > 0.f && d->keep_in <= 1.f && d->keep_out > 0.f && d->keep_out <= 1.f,
                 "lstm: keep probabilities must be in (0,1]");
    AS_CHECK_ARG((size_t)d->T * d->B * d->H < (1ull << 32), "lstm: T*B*H too large for the dropout counter");
    AS_CHECK_ARG(d->precision == 0 || ((d->precision == 1 || d->precision == 2) && d->H % 32 == 0),
                 "lstm: precision %d unsupported (0 = f32; 1 = bf16x3, 2 = bf16: both need H %% 32 == 0, H = %d)", d->precision, d->H);
    AS_CHECK_ARG((d->flags & ~(AMDSPEECH_LSTM_ARMED | AMDSPEECH_LSTM_ARM_NEXT | AMDSPEECH_LSTM_SAME_WS | AMDSPEECH_LSTM_PER_DIAGONAL |
                               AMDSPEECH_LSTM_INJECT_TIMEOUT)) == 0, "lstm: unknown flags 0x%x", d->flags);
    return AMDSPEECH_OK;
}

// ------------------------------------------------------------------- dropout
struct DropCfg { float keep_in, keep_out; uint64_t seed; int L; };

// Multiplier of inter-layer tensor Z_lp (lp = 0..L): input mask of layer lp (if it
// exists) times output mask of layer lp-1 (if it exists), each mask/keep.
__device__ __forceinline__ float zmult(const DropCfg& c, int lp, uint32_t idx) {
    float m = 1.0f;
    if (c.keep_in < 1.0f && lp < c.L)
        m *= (uniform01(c.seed, 2u * lp, idx) < c.keep_in) ? (1.0f / c.keep_in) : 0.0f;
    if (c.keep_out < 1.0f && lp >= 1)
        m *= (uniform01(c.seed, 2u * (lp - 1) + 1u, idx) < c.keep_out) ? (1.0f / c.keep_out) : 0.0f;
    return m;
}

__global__ void apply_zmult_kernel(float* x, long n, DropCfg c, int lp) {
    long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) x[i] *= zmult(c, lp, (uint32_t)i);
}

// ------------------------------------------------------------ weight packing
// Forward B-fragments.  Workgroup ub owns UW units x 4 gates = 4*UW columns,
// local column c = g*UW + u, N-tile nt = c/16, j = c%16.  For K-block kb (16 rows
// of K) lane (j, kq) holds rows kb*16 + 4*kq + m, m = 0..3, as one float4:
//   Wp[(((l*NUB + ub)*NKB + kb)*NT + nt)*256 + lane*4 + m]
// grouped != 0 (persistent kernel): every N tile holds all four gates of 4 units instead,
//   unit u = nt*4 + j%4, gate g = j/4.
__global__ void pack_fwd_kernel(const float* __restrict__ kernels, long kstride, float* __restrict__ wp,
                                int H, int L, int UW, int grouped) {
    const int NT = UW / 4, NKB = 2 * H / 16, NUB = H / UW;
    const long total = (long)L * 2 * H * 4 * H;
    long o = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (o >= total) return;
    int m = o & 3, lane = (o >> 2) & 63;
    long r = o >> 8;
    int nt = r % NT; r /= NT;
    int kb = r % NKB; r /= NKB;
    int ub = r % NUB; int l = r / NUB;
    int j = lane & 15, kq = lane >> 4;
    int c = nt * 16 + j, g = c / UW, u = c % UW;
    if (grouped) { g = j >> 2; u = nt * 4 + (j & 3); }
    int k = kb * 16 + 4 * kq + m;
    wp[o] = kernels[l * kstride + (long)k * 4 * H + g * H + ub * UW + u];
}

// Backward B-fragments = K^T: row block rb (16 rows of K = 16 input units), K-block
// kb (16 gate columns):  Wq[((l*(2H/16) + rb)*(4H/16) + kb)*256 + lane*4 + m]
//   = K_l[rb*16 + (lane&15)][kb*16 + 4*(lane>>4) + m]
__global__ void pack_bwd_kernel(const float* __restrict__ kernels, long kstride, float* __restrict__ wq,
                                int H, int L) {
    const int NRB = 2 * H / 16, NKB = 4 * H / 16;
    const long total = (long)L * 2 * H * 4 * H;
    long o = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (o >= total) return;
    int m = o & 3, lane = (o >> 2) & 63;
    long r = o >> 8;
    int kb = r % NKB; r /= NKB;
    int rb = r % NRB; int l = r / NRB;
    int row = rb * 16 + (lane & 15), col = kb * 16 + 4 * (lane >> 4) + m;
    wq[o] = kernels[l * kstride + (long)row * 4 * H + col];
}

// Fragment-major layout of a [rows, K] panel (rows padded to 16): tile (mt = row/16, kb = k/16)
// is one 1 KiB block ordered [lane][m] with lane = ((k/4)%4)*16 + row%16, m = k%4 -- exactly the
// v_mfma_f32_16x16x4_f32 A operand of four consecutive MFMAs, so a wave reads it with ONE fully
// coalesced float4 load instead of touching 16 rows.
__device__ __forceinline__ size_t packed_off(int row, int k, int K) {
    return ((((size_t)(row >> 4) * (K >> 4) + (k >> 4)) * 64) + (((k >> 2) & 3) * 16 + (row & 15))) * 4 + (k & 3);
}

// src: nmat row-major [B][K] panels (stride src_stride) -> dst: nmat packed panels (stride bp*K)
__global__ void pack_rows_kernel(const float* __restrict__ src, size_t src_stride, float* __restrict__ dst,
                                 int B, int K, int nmat) {
    const size_t per = (size_t)B * K;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= per * nmat) return;
    const int mat = i / per;
    const size_t r = i % per;
    const int row = r / K, k = r % K;
    const size_t bpk = (size_t)((B + 15) / 16 * 16) * K;
    dst[(size_t)mat * bpk + packed_off(row, k, K)] = src[(size_t)mat * src_stride + r];
}

// Layer-0 input of the dataflow forward kernel in one pass: Z_0 *= input-dropout multiplier (in place: the backward pass
// reads the masked Z_0) and the packed panels of all T frames.  One thread = four consecutive features of one row.
__global__ __launch_bounds__(256) void mask_pack_rows_kernel(float* __restrict__ z, float* __restrict__ dst, int B, int K, int T,
                                                             DropCfg c, int masked) {
    const size_t per4 = (size_t)B * K / 4;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= per4 * T) return;
    const int t = i / per4;
    const size_t r = (i % per4) * 4;
    const int row = r / K, k = r % K;
    const size_t e = (size_t)t * B * K + r;
    float4 v = *reinterpret_cast<const float4*>(z + e);
    if (masked) {
        v.x *= zmult(c, 0, (uint32_t)e); v.y *= zmult(c, 0, (uint32_t)(e + 1));
        v.z *= zmult(c, 0, (uint32_t)(e + 2)); v.w *= zmult(c, 0, (uint32_t)(e + 3));
        *reinterpret_cast<float4*>(z + e) = v;
    }
    const size_t bpk = (size_t)((B + 15) / 16 * 16) * K;
    *reinterpret_cast<float4*>(dst + (size_t)t * bpk + packed_off(row, k, K)) = v;
}

// Everything small the dataflow forward kernel needs before it starts, in one launch: the initial state rows hs[l][0] /
// cs[l][0] (given, or zeros), the packed h_{-1} panels (slot 0 of hph, padding rows zero), the error word and the tickets.
__global__ __launch_bounds__(256) void flow_fwd_prepare_kernel(const float* __restrict__ h0, const float* __restrict__ c0,
                                                               float* __restrict__ hs, float* __restrict__ cs,
                                                               float* __restrict__ hph, unsigned* __restrict__ sync_words,
                                                               int T, int B, int H, int L) {
    const int bp = (B + 15) / 16 * 16;
    const size_t per = (size_t)bp * H;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < 40) sync_words[i] = 0u;              // error word (+ progress words), the per-XCD tickets
    if (i >= per * L) return;
    const int l = i / per;
    const size_t r = i % per;
    const int row = r / H, k = r % H;
    float hv = 0.f;
    if (row < B) {
        const size_t e = (size_t)row * H + k, bh = (size_t)B * H;
        hv = h0 ? h0[l * bh + e] : 0.f;
        hs[(size_t)l * (T + 1) * bh + e] = hv;
        cs[(size_t)l * (T + 1) * bh + e] = c0 ? c0[l * bh + e] : 0.f;
    }
    hph[(size_t)l * (T + 1) * per + packed_off(row, k, H)] = hv;
}

__device__ __forceinline__ float sigmoidf_(float x) { return 1.0f / (1.0f + expf(-x)); }

#include "lstm_step_fwd.h"
#include "lstm_flow.h"
}  // namespace amdspeech
#include "ctc_flow.h"      // the CTC head inside the dataflow kernels (needs FLOW_SENTINEL / flow_pending above)
namespace amdspeech {

#include "lstm_flow_fwd.h"
#include "lstm_big_fwd.h"
#include "lstm_step_bwd.h"
#include "lstm_flow_bwd.h"
#include "lstm_big_bwd.h"
#include "lstm_step_bf3.h"
// ---------------------------------------------------------------- profiling
// HIP-event time of the recurrence kernels of the last call, per direction.  The per-layer paths (H = 1024) launch one kernel
// per layer with GEMMs in between: every kernel gets its own event pair (a "segment") and the reported time is their sum.
constexpr int PROF_SEGS = 16;
static bool g_prof_on = false;
static hipEvent_t g_prof_ev[2][PROF_SEGS][2];
static int g_prof_launches[2] = {0, 0};
static int g_prof_nseg[2] = {0, 0};
static bool g_prof_valid[2] = {false, false};
static double g_prof_flops[2][2] = {{0, 0}, {0, 0}};      // [which][0: recurrence products, 1: other products inside the same launches]
static void prof_flops(int which, double recurrence, double other) { g_prof_flops[which][0] = recurrence; g_prof_flops[which][1] = other; }

static void prof_begin(int which, hipStream_t s, int seg = 0) {
    if (g_prof_on && seg < PROF_SEGS) (void)hipEventRecord(g_prof_ev[which][seg][0], s);
}
static void prof_end(int which, hipStream_t s, int launches, int seg = 0) {
    if (!g_prof_on || seg >= PROF_SEGS) return;
    (void)hipEventRecord(g_prof_ev[which][seg][1], s);
    g_prof_launches[which] = launches;
    g_prof_nseg[which] = seg + 1;
    g_prof_valid[which] = true;
}

// The side stream the fills for the next call go out on (AMDSPEECH_LSTM_ARM_NEXT)
static hipStream_t g_side = nullptr;
static hipEvent_t g_fork = nullptr;
static int side_stream_init() {
    if (g_side) return AMDSPEECH_OK;
    AS_CHECK_HIP(hipStreamCreateWithFlags(&g_side, hipStreamNonBlocking));
    AS_CHECK_HIP(hipEventCreateWithFlags(&g_fork, hipEventDisableTiming));
    return AMDSPEECH_OK;
}
// Weight-gradient GEMMs of finished time chunks of the per-diagonal backward pass run on the side stream UNDER the rest of the
// BPTT chain (the chain leaves 64 CUs idle and the MFMA pipes mostly free).
// CU partition (hipExtStreamCreateWithCUMask; mask bit i = CU i/8 of XCD i%8 on this part, measured with
// tools/cumask_probe.hip): the chain gets 24 CUs of every XCD (its grids are 192 workgroups anyway), the GEMMs
// the other 8 -- un-partitioned, the MFMA-saturating GEMM waves share SIMDs with the chain's and make every
// diagonal 1.7x slower, which cancels the overlap.
static hipStream_t g_chain = nullptr, g_gemm = nullptr;
static hipEvent_t g_ev_a = nullptr, g_ev_b = nullptr, g_ev_c = nullptr;
static int g_overlap_state = 0;      // 0 = not tried, 1 = ready, -1 = unavailable on this device
static int overlap_init() {
    if (g_overlap_state != 0) return g_overlap_state;
    g_overlap_state = -1;
    int dev = 0, cus = 0;
    if (hipGetDevice(&dev) != hipSuccess) return -1;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus != 256) return -1;
    uint32_t chain_mask[8] = {0, 0, ~0u, ~0u, ~0u, ~0u, ~0u, ~0u}, gemm_mask[8] = {~0u, ~0u, 0, 0, 0, 0, 0, 0};
    if (hipExtStreamCreateWithCUMask(&g_chain, 8, chain_mask) != hipSuccess) return -1;
    if (hipExtStreamCreateWithCUMask(&g_gemm, 8, gemm_mask) != hipSuccess) return -1;
    if (hipEventCreateWithFlags(&g_ev_a, hipEventDisableTiming) != hipSuccess) return -1;
    if (hipEventCreateWithFlags(&g_ev_b, hipEventDisableTiming) != hipSuccess) return -1;
    if (hipEventCreateWithFlags(&g_ev_c, hipEventDisableTiming) != hipSuccess) return -1;
    g_overlap_state = 1;
    return 1;
}
// The T axis is cut into DK_CHUNKS pieces; the first DK_SIDE of them (in the order the chain finishes them) run on the GEMM
// partition under the chain, the rest after it on the whole chip.
constexpr int DK_CHUNKS = 8, DK_SIDE = 5;

// --------------------------------------------------------------- host side
// precision = bf16x3 / bf16 also covers the BATCHED products around the recurrence (round 3; gemm_bf3.hip): the hoisted x . W_ih and
// dX = dG . W_ih^T of the H = 1024 path, the weight gradients and dZ_0 of every path -- through the GEMM of that precision (1: three
// bf16 MFMAs per product, 2: one)
static int gemm_reduced(const amdspeech_lstm_desc* d, hipStream_t s, bool ta, bool tb, int M, int N, int K, const float* A, int lda,
                        const float* B, int ldb, float* C, int ldc, const float* bias, bool accumulate) {
    return (d->precision == 2 ? gemm_bf16 : gemm_bf3)(s, ta, tb, M, N, K, A, lda, B, ldb, C, ldc, bias, accumulate);
}
// ... a batched product in the descriptor's precision
static int gemm_batched(const amdspeech_lstm_desc* d, hipStream_t s, bool ta, bool tb, int M, int N, int K, const float* A, int lda,
                        const float* B, int ldb, float* C, int ldc, const float* bias, bool accumulate) {
    if (d->precision != 0) return gemm_reduced(d, s, ta, tb, M, N, K, A, lda, B, ldb, C, ldc, bias, accumulate);
    return gemm_f32(s, ta, tb, M, N, K, A, lda, B, ldb, C, ldc, bias, accumulate);
}
static int pick_uw(const amdspeech_lstm_desc* d) {
    // 8 units (two 16-column N tiles) per workgroup halves the redundant re-reads of the
    // [B, 2H] activation panel; fall back to 4 when that would leave most CUs without work.
    const long wgs8 = (long)d->L * (d->H / 8) * ceil_div(d->B, 32);
    return (d->H % 8 == 0 && wgs8 >= 96) ? 8 : 4;
}

static int device_cus() {
    static int cus = -1;
    if (cus < 0) {
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess ||
            hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) cus = 0;
    }
    return cus;
}

// H = 1024 forward: one weight-stationary launch per layer (lstm_fwd_big); AMDSPEECH_BIG=0 turns it off
static bool use_big_fwd(const amdspeech_lstm_desc* d) {
    static const int env = runtime_switch("AMDSPEECH_BIG", 1);
    // (AMDSPEECH_LSTM_PER_DIAGONAL: the re-run of a mini-batch whose launch gave up waiting takes NO kernel with bounded waits)
    return env != 0 && !(d->flags & AMDSPEECH_LSTM_PER_DIAGONAL) && d->precision >= 0 && d->precision <= 2 && d->H == 1024 &&
           (d->B + 15) / 16 <= 4 && device_cus() == 256 &&
           (size_t)2 * ((d->B + 15) / 16 * 16) * d->H * 4 < (1ull << 32);
}

// AMDSPEECH_FLOW=0 falls back to one launch per diagonal
static bool use_flow(const amdspeech_lstm_desc* d) {
    static const int env = runtime_switch("AMDSPEECH_FLOW", 1);
    // (8 XCDs x 32 CUs: the backward kernel places one recurrence group per XCD)
    // (AMDSPEECH_LSTM_PER_DIAGONAL: this call asks for the launch-per-diagonal kernels -- the re-run of a mini-batch whose dataflow
    //  launch timed out; the workspace layout does not depend on it)
    return env != 0 && !(d->flags & AMDSPEECH_LSTM_PER_DIAGONAL) && flow_shape_ok(d) && device_cus() == 256 && d->L * ((d->B + 15) / 16) <= 8;
}

// The instantiations of the two dataflow kernels, by K blocks per wave and half (H / 128) and precision; CF: with the fused CTC
// head's role (flow_shape_ok: reduced precision only at H = 256, 512; x-product workers only in exact f32 at H = 512)
template <bool CF>
static void (*flow_fwd_kernel(int kb, int pr, int mv, int mh, int me))(FlowArgs) {
    switch (kb) {
        case 1: return lstm_fwd_flow2<1, 0, 0, CF>;
        case 2: return pr == 2 ? lstm_fwd_flow2<2, 2, 0, CF> : (pr == 1 ? lstm_fwd_flow2<2, 1, 0, CF> : lstm_fwd_flow2<2, 0, 0, CF>);
        case 3: return lstm_fwd_flow2<3, 0, 0, CF>;
        default:
            if (pr == 0 && mv == 1 && mh == 1) return me > 0 ? lstm_fwd_flow2<4, 0, 1, CF, 1, FWD2_HALF_KSTEPS> : lstm_fwd_flow2<4, 0, 1, CF, 1>;
            if (pr == 0 && mv == 1) return lstm_fwd_flow2<4, 0, 1, CF>;
            return pr == 2 ? lstm_fwd_flow2<4, 2, 0, CF> : (pr == 1 ? lstm_fwd_flow2<4, 1, 0, CF> : lstm_fwd_flow2<4, 0, 0, CF>);
    }
}
template <bool CF>
static void (*flow_bwd_kernel(int kb, int pr))(FlowBwdArgs) {
    if (pr == 2) return kb == 2 ? lstm_bwd_flow2<2, 2, CF> : lstm_bwd_flow2<4, 2, CF>;
    if (pr == 1) return kb == 2 ? lstm_bwd_flow2<2, 1, CF> : lstm_bwd_flow2<4, 1, CF>;
    return kb == 1 ? lstm_bwd_flow2<1, 0, CF> : (kb == 2 ? lstm_bwd_flow2<2, 0, CF> : (kb == 3 ? lstm_bwd_flow2<3, 0, CF> : lstm_bwd_flow2<4, 0, CF>));
}
// ---- the panels the dataflow kernels poll (amdspeech.h: AMDSPEECH_LSTM_ARMED / ARM_NEXT)
// forward: sentinel in every slot the kernel will write (each exactly once; layer 0 reads xp0, not xph[0])
static int flow_fill_fwd_panels(hipStream_t s, const amdspeech_lstm_desc* d, float* ws, const LstmLayout& lo, int set) {
    const size_t bph = (size_t)(d->B + 15) / 16 * 16 * d->H;
    float* base = ws + (size_t)set * lo.fwd_set;
    // (slot [L]: the top layer's output panels, polled by the fused CTC head -- filled whether or not this call has one: the set
    //  is armed for the NEXT call, whose head is not known yet)
    AS_CHECK_HIP(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(base + lo.xph + (size_t)d->T * bph), (int)FLOW_SENTINEL,
                                   (size_t)d->L * d->T * bph, s));
    AS_CHECK_HIP(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(base + lo.hph), (int)FLOW_SENTINEL, (size_t)d->L * (d->T + 1) * bph, s));
    return AMDSPEECH_OK;
}
// backward: the dG panels (round-1 kernel) or the two partial-tile rings (parity 0), and the dX panels between the layers
static int flow_fill_bwd_panels(hipStream_t s, const amdspeech_lstm_desc* d, float* ws, const LstmLayout& lo, bool ctc_head = false) {
    const size_t bpg = (size_t)((d->B + 15) / 16) * 16 * 4 * d->H;
    AS_CHECK_HIP(hipMemsetAsync(ws + lo.prec, 0, (lo.total - lo.prec) * sizeof(float), s));
    if (ctc_head)      // dZ_top is produced DURING the backward launch (ctc_leader) and polled by the top layer's groups
        AS_CHECK_HIP(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(ws + lo.dztop), (int)FLOW_SENTINEL, (size_t)d->T * d->B * d->H, s));
    if (d->L > 1)
        AS_CHECK_HIP(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(ws + lo.dxh), (int)FLOW_SENTINEL,
                                       (size_t)(d->L - 1) * d->T * (bpg / 4), s));
    return AMDSPEECH_OK;
}
// Side-stream fills: flow_arm_fork orders the side stream behind everything enqueued on `s` so far; the fills enqueued on it
// since are "pending" until some later lstm call makes its stream wait for them (flow_arm_settle: every dataflow call does)
// The pending state belongs to the WORKSPACE the fills write into (keyed by its base address; amdspeech_lstm_workspace_release
// forgets it): two engines -- or the two stacks of a bidirectional model -- never wait for each other's fills.
struct ArmState {
    hipEvent_t join = nullptr; bool pending = false;
    // amdspeech_lstm_beside_forward: recorded on the caller's stream just in front of the last forward dataflow launch on this
    // workspace; idle_xcds = how many XCDs that launch leaves without a recurrence group
    hipEvent_t pre = nullptr; int idle_xcds = 0;
    // amdspeech_lstm_beside_tail: recorded just behind the last backward dataflow launch on this workspace (in front of the
    // weight-gradient launches that follow it); post_flags: 1 = recorded, 2 = dZ_0 is complete at that point
    hipEvent_t post = nullptr; int post_flags = 0;
    int clean_set = 0;      // the set of forward panels an ARMED forward call finds prepared
    int xw_par = -1;        // the tag (0 / 1) the last forward launch left in EVERY word of the x-product workers' tile history it
                            // wrote; -1: unknown (the next launch zeroes the history and uses 1)
    int xw_cover = 0;       // ... and the number of leading frames that carry it (that launch's T)
    long xw_key = 0;        // ... at this shape (B, H, L, parts)
};
static std::mutex g_arm_mutex;
static std::unordered_map<const void*, ArmState> g_arm;
// The tag of this launch's tiles.  A call that may trust the history (ARMED / SAME_WS, amdspeech.h: the previous lstm_fwd on this
// workspace ran at the same B / H / L and nothing else has written to it) flips the tag the previous launch left in frames
// [0, cover) and, when it runs more frames than that launch, gives the frames [cover, T) the OLD tag first (they may hold either:
// a shorter launch in between left them alone); any other call zeroes the frames it will use (0.8 GB per part at the benchmark
// shape: once per training run).
static int flow_xw_parity(hipStream_t s, const void* ws, bool trust, long key, float* xwp, size_t frame_floats, int T, unsigned* par) {
    std::lock_guard<std::mutex> lock(g_arm_mutex);
    ArmState& st = g_arm[ws];
    if (trust && st.xw_par >= 0 && st.xw_key == key) {
        const int old = st.xw_par;
        if (T > st.xw_cover)
            AS_CHECK_HIP(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(xwp + (size_t)st.xw_cover * frame_floats), old,
                                           (size_t)(T - st.xw_cover) * frame_floats, s));
        st.xw_par = old ^ 1;
    } else {
        AS_CHECK_HIP(hipMemsetAsync(xwp, 0, (size_t)T * frame_floats * sizeof(float), s));
        st.xw_par = 1;
    }
    st.xw_cover = T; st.xw_key = key;
    *par = (unsigned)st.xw_par;
    return AMDSPEECH_OK;
}
static void flow_xw_forget(const void* ws) {      // (a launch that did not complete: its tiles carry either tag)
    std::lock_guard<std::mutex> lock(g_arm_mutex);
    auto it = g_arm.find(ws);
    if (it != g_arm.end()) it->second.xw_par = -1;
}
static int flow_arm_fork(hipStream_t s) {
    if (int rc = side_stream_init()) return rc;
    AS_CHECK_HIP(hipEventRecord(g_fork, s));
    AS_CHECK_HIP(hipStreamWaitEvent(g_side, g_fork, 0));
    return AMDSPEECH_OK;
}
static int flow_clean_set(const void* ws) {
    std::lock_guard<std::mutex> lock(g_arm_mutex);
    auto it = g_arm.find(ws);
    return it == g_arm.end() ? 0 : it->second.clean_set;
}
static int flow_arm_publish(const void* ws, int clean_set) {
    std::lock_guard<std::mutex> lock(g_arm_mutex);
    ArmState& st = g_arm[ws];
    st.clean_set = clean_set;
    if (!st.join) AS_CHECK_HIP(hipEventCreateWithFlags(&st.join, hipEventDisableTiming));
    AS_CHECK_HIP(hipEventRecord(st.join, g_side));
    st.pending = true;
    return AMDSPEECH_OK;
}
static int flow_arm_settle(hipStream_t s, const void* ws) {
    std::lock_guard<std::mutex> lock(g_arm_mutex);
    auto it = g_arm.find(ws);
    if (it == g_arm.end() || !it->second.pending) return AMDSPEECH_OK;
    AS_CHECK_HIP(hipStreamWaitEvent(s, it->second.join, 0));
    it->second.pending = false;
    return AMDSPEECH_OK;
}
static int flow_arm_release(hipStream_t s, const void* ws) {
    std::lock_guard<std::mutex> lock(g_arm_mutex);
    auto it = g_arm.find(ws);
    if (it == g_arm.end()) return AMDSPEECH_OK;
    if (it->second.pending) AS_CHECK_HIP(hipStreamWaitEvent(s, it->second.join, 0));
    if (it->second.join) (void)hipEventDestroy(it->second.join);
    if (it->second.pre) (void)hipEventDestroy(it->second.pre);
    if (it->second.post) (void)hipEventDestroy(it->second.post);
    g_arm.erase(it);
    return AMDSPEECH_OK;
}
// the point in stream `s` just in front of a forward launch on `ws` (idle_xcds = 0: a launch that leaves nothing idle)
static int flow_mark_postlaunch(hipStream_t s, const void* ws, int flags) {
    std::lock_guard<std::mutex> lock(g_arm_mutex);
    ArmState& st = g_arm[ws];
    st.post_flags = flags;
    if (flags == 0) return AMDSPEECH_OK;
    if (!st.post) AS_CHECK_HIP(hipEventCreateWithFlags(&st.post, hipEventDisableTiming));
    AS_CHECK_HIP(hipEventRecord(st.post, s));
    return AMDSPEECH_OK;
}
static int flow_mark_prelaunch(hipStream_t s, const void* ws, int idle_xcds) {
    std::lock_guard<std::mutex> lock(g_arm_mutex);
    ArmState& st = g_arm[ws];
    st.idle_xcds = idle_xcds;
    if (idle_xcds <= 0) return AMDSPEECH_OK;
    if (!st.pre) AS_CHECK_HIP(hipEventCreateWithFlags(&st.pre, hipEventDisableTiming));
    AS_CHECK_HIP(hipEventRecord(st.pre, s));
    return AMDSPEECH_OK;
}

// The fused CTC head (amdspeech.h: amdspeech_lstm_ctc_fusable) on a dataflow shape: how many workgroups of every spare XCD follow
// the forward recurrence (behind the wpx x-product workers; the rest stay free for side-stream work), 0 = the shape does not take it
static int ctc_head_nfw(const amdspeech_lstm_desc* d, int C, int U, int wpx) {
    static const int env = runtime_switch("AMDSPEECH_FLOW_CTC", 1);      // 0: the CTC stage as launches between the two recurrence kernels
    if (env == 0) return 0;
    const int groups = d->L * ((d->B + 15) / 16), spare = 8 - groups, smax = 2 * U + 1;
    if (spare < 1 || C < 16 || C > 16 * CF_NTC || C % 16 != 0 || U < 1 || smax > 384 || d->H % 64 != 0) return 0;
    if ((size_t)d->B * d->T * smax * 4 >= (1ull << 31) || (size_t)d->T * d->B * d->H * 4 >= (1ull << 31)) return 0;
    int nfw = 32 - wpx < 4 ? 32 - wpx : 4;
    if (nfw < 1 || d->B > spare * nfw * 2 * 2) return 0;      // at most two utterances per team
    return nfw;
}
static CtcFlow ctc_head_args(const amdspeech_lstm_desc* d, const amdspeech_ctc_head* h, float* ws, const LstmLayout& lo, float* panels, int nfw) {
    const CtcLayout cl = ctc_layout(d->T, d->B, h->C, h->U);
    char* w = static_cast<char*>(h->ctc_ws);
    CtcFlow c;
    c.on = 1; c.C = h->C; c.smax = cl.smax; c.nfw = nfw; c.T = d->T; c.B = d->B;
    c.ztp = panels ? panels + lo.xph + (size_t)d->L * d->T * ((size_t)(d->B + 15) / 16 * 16 * d->H) : nullptr;
    c.wo = h->w_out; c.wo_pack = ws + lo.wopack; c.bo = h->b_out;
    c.logits = h->logits; c.logp = reinterpret_cast<float*>(w + cl.logp); c.alpha = reinterpret_cast<float*>(w + cl.alpha);
    c.ll = reinterpret_cast<float*>(w + cl.ll); c.loss = h->loss; c.dlogits = h->dlogits; c.dztop = ws + lo.dztop;
    c.ext = reinterpret_cast<const int*>(w + cl.ext); c.slen = reinterpret_cast<const int*>(w + cl.slen);
    c.valid = reinterpret_cast<const int*>(w + cl.valid);
    return c;
}

// ------------------------------------------------------------------- the plan of one call
// Every kernel-path decision of a call, made once from the descriptor (and the fused CTC head, if any): the workspace layout, the
// size and fusability queries and both directions read it and derive none of it again.
enum class Path {
    flow,        // one launch per sequence and direction (lstm_fwd_flow2 / lstm_bwd_flow2)
    big1,        // H = 1024, one launch per layer on the one-XCD groups (lstm_fwd_big1 / lstm_bwd_big1)
    big,         // H = 1024, one launch per layer on the XCD pairs (lstm_fwd_big / lstm_bwd_big)
    hoist,       // backward only: one launch per frame and layer, the gradient for the layer below by one GEMM per layer
    diag,        // one launch per diagonal (lstm_fwd_step / lstm_bwd_step)
    diag_bf3,    // ... in bf16x3 (lstm_fwd_step_bf3 / lstm_bwd_step_bf3)
};
struct LstmPlan {
    amdspeech_lstm_desc d;
    int nmt;                              // 16-row batch tiles
    // what the workspace reserves
    bool flow_shape;                      // the panels and rings of the dataflow kernels
    int xw_parts;                         // ... and the x-product workers' tile history: K blocks per recurrence wave (0 or 1)
    int xw_half;                          // ... and the half roles' tiles in every frame of it (0 or 1: fwd_half_roles_fit)
    bool big_ring;                        // the rings of lstm_bwd_big / lstm_bwd_big1
    bool bf16p_reserved;                  // the bf16 operand copies of the batched products (gemm_bf16p.hip) ...
    bool bf16p;                           // ... and whether this T uses them
    // the paths and their kernels
    Path fwd, bwd;
    bool pair;                            // two stacks of this shape run side by side (amdspeech_lstm_pair_fusable)
    int uw;                               // units per workgroup of the forward weight pack
    unsigned long long limit;             // bound on the waits of the dataflow and per-layer kernels (100 MHz ticks)
    void (*fwd_diag)(FwdArgs); int fwd_mt;                // (lstm_fwd_step: 16-row M tiles per workgroup)
    void (*bwd_diag)(BwdArgs);                            // (the hoisted backward too)
    void (*fwd_big)(BigFwdArgs); void (*bwd_big)(BigBwdArgs);
    void (*fwd_flow)(FlowArgs); void (*bwd_flow)(FlowBwdArgs);
    size_t fwd_lds, bwd_lds;              // their dynamic LDS
    int mv, wpx, wpw;                     // x-product workers: K blocks per recurrence wave (0: none), workgroups per spare XCD, waves per role
    int mh;                               // ... half roles on waves 4-7 of those workgroups (0 or 1; wpw = 4 then)
    int me;                               // ... the k-steps of the block below that the half roles take as well (0, or FWD2_HALF_KSTEPS)
    int nfw;                             // the fused CTC head's followers per spare XCD (0: no head, or the shape does not take it)
    int dz0_inkernel;                     // lstm_bwd_flow2: dZ_0 formed by the layer-0 groups
    int w_pieces, w_t0, w_dz0;            // ... its in-kernel weight gradients: chunks (0: none), first frame, dZ_0 too
    bool w_deal;                          // ... dealt from counters
};

// AMDSPEECH_FLOW_GEMM = "pieces:percent" (development builds; tools/share_sweep.sh): the weight-gradient GEMMs of the LAST `percent` %
// of the frames (the first the recurrence finishes) are computed INSIDE lstm_bwd_flow2, in `pieces` chunks, by the workgroups of
// the XCDs that carry no recurrence group (bwd_gemm_worker); 0:0 leaves all of them to the launches behind it.
struct FlowGemmShare { int pieces, percent; bool set; };
static FlowGemmShare flow_gemm_share() {
    static const FlowGemmShare g = [] {
        // measured at cfg2 with lstm_bwd_flow2 and the LDS-free worker tiles (dK only, see w_dz0): ms per step at 28 / 34 / 40 /
        // 44 / 48 % = 16.04 / 15.69 / 15.44-15.73 / 15.93 / 16.32 -- past ~40 % the kernel waits for its workers, steeply
        // round 6 (Q = 4 kernel, fused head, pieces:percent -> ms per step, two alternations on one box): 4:35 12.02 / 11.98, 8:38 11.92 /
        // 11.93, 8:40 12.14 / 12.13, 8:42 12.29, 6:40 12.15 -- eight chunks release the first frames to the workers 0.24 ms earlier
        FlowGemmShare r{8, 38, false};
        if (const char* e = dev_knob_str("AMDSPEECH_FLOW_GEMM")) {
            r.set = true;
            r.pieces = atoi(e);
            if (const char* q = strchr(e, ':')) r.percent = atoi(q + 1);
        }
        if (r.pieces < 0) r.pieces = 0;
        if (r.percent < 0) r.percent = 0;
        if (r.percent > 90) r.percent = 90;
        return r;
    }();
    return g;
}

static LstmPlan lstm_plan(const amdspeech_lstm_desc* d, const amdspeech_ctc_head* head) {
    LstmPlan p{};
    p.d = *d;
    const int T = d->T, H = d->H, L = d->L, pr = d->precision;
    p.nmt = (d->B + 15) / 16;
    p.flow_shape = flow_shape_ok(d);
    p.xw_parts = p.flow_shape && fwd_workers_fit(d) ? 1 : 0;
    p.xw_half = p.xw_parts > 0 && fwd_half_roles_fit(d) ? 1 : 0;
    p.big_ring = !p.flow_shape && pr >= 0 && pr <= 2 && H == 1024 && p.nmt <= 4;
    p.bf16p_reserved = bf16p_layout_reserved(d);
    p.bf16p = bf16p_layout_on(d);
    // generous bound on the whole sequence: 100 us per step plus a second (AMDSPEECH_LSTM_INJECT_TIMEOUT: tests)
    p.limit = (d->flags & AMDSPEECH_LSTM_INJECT_TIMEOUT) ? 0ull : 100000000ull + (unsigned long long)T * 10000ull;

    // ---- the paths.  H = 1024 in plain bf16: a batch tile's group fits ONE XCD (lstm_fwd_big1 / lstm_bwd_big1), and two stacks of one
    // shape run side by side on the two halves of the chip (amdspeech_lstm_fwd_pair / _bwd_pair); AMDSPEECH_BIG1=0: one after the
    // other on the XCD pairs.  One stack alone runs forward on the XCD pairs -- 13.3 against 14.7 ms of recurrence at configs[2]'s
    // shape, half the MFMAs and half the LDS traffic per CU and step; AMDSPEECH_BIG1=2 runs it on the one-XCD groups all the same --
    // and backward on the one-XCD groups (the faster backward kernel, see lstm_big_bwd.h) whenever the bf16 operand copies are used.
    static const int big1_env = runtime_switch("AMDSPEECH_BIG1", 1);
    const bool flow = use_flow(d), big = !flow && use_big_fwd(d);
    p.pair = big && big1_env != 0 && pr == 2;
    // (precision 2 outside the dataflow / per-layer shapes: the bf16x3 step kernels, a superset in accuracy; the dataflow and per-layer
    //  kernels split their f32 fragments in registers: f32 packs)
    const Path diag = pr != 0 ? Path::diag_bf3 : Path::diag;
    p.fwd = flow ? Path::flow : big ? (p.pair && big1_env == 2 ? Path::big1 : Path::big) : diag;
    // Shapes whose weights do not fit on chip (H >= 768) run the backward pass layer by layer with the time-independent half of every
    // product HOISTED out of the recurrence: dX_{l-1} = dG_l.W_ih^T for all frames once layer l is done (the per-frame kernel keeps
    // only the recurrent product).  Measured (5x1024, B = 64, T = 998): the backward pass gains (147 -> 129 ms); the forward pass does
    // not (82 ms either way: a launch per frame and layer costs what a launch per diagonal of five layers saved), and with ONE batch
    // tile (3x1024, B = 10) tripling the launch count loses (179 -> 237 ms).
    p.bwd = flow ? Path::flow : (p.pair && p.bf16p) ? Path::big1 : big ? Path::big
          : (pr == 0 && H >= 768 && p.nmt >= 2) ? Path::hoist : diag;
    p.uw = (flow || big) ? 16 : pick_uw(d);      // the dataflow and per-layer kernels own 16 units x 4 gates per workgroup

    // ---- the kernels
    p.fwd_mt = p.nmt % 2 == 0 ? 2 : 1;
    if (pr != 0) p.fwd_diag = lstm_fwd_step_bf3<8>;
    else if (p.uw == 8) p.fwd_diag = p.fwd_mt == 2 ? lstm_fwd_step<8, 8, 8, false, 2> : lstm_fwd_step<8, 8, 8, false, 1>;
    else p.fwd_diag = p.fwd_mt == 2 ? lstm_fwd_step<4, 8, 8, false, 2> : lstm_fwd_step<4, 8, 8, false, 1>;
    p.bwd_diag = pr != 0 ? lstm_bwd_step_bf3<8> : lstm_bwd_step<8, 8, true>;
    p.fwd_big = pr == 2 ? lstm_fwd_big<2> : (pr == 1 ? lstm_fwd_big<1> : lstm_fwd_big<0>);
    p.bwd_big = pr == 2 ? lstm_bwd_big<2> : (pr == 1 ? lstm_bwd_big<1> : lstm_bwd_big<0>);
    if (!flow) return p;

    // ---- the dataflow kernels.  x-product workers (lstm_fwd_flow2<., ., 1>): one role per SIMD where that fits, else two; where one
    // fits, waves 4-7 of the worker workgroups take half roles (lstm_fwd_flow2<., ., 1, ., 1>: a block and a half per recurrence wave)
    // (AMDSPEECH_FLOW_FWD_WORKERS=0: the kernel of rounds 2 - 4, every recurrence wave multiplies its whole x half; 1: full roles only;
    //  2: full and half roles, the half roles without the k-steps of the block below -- the kernel of round 6; unset / 3: with them)
    static const int workers_env = runtime_switch("AMDSPEECH_FLOW_FWD_WORKERS", 3);
    const int groups = L * p.nmt, spare = 8 - groups;
    p.wpw = 8;
    if (workers_env != 0 && p.xw_parts > 0)
        for (int waves = 4; waves <= 8 && p.mv == 0; waves += 4) {
            const int per = fwd_worker_wgs_per_xcd(d, waves);
            if (per <= 32 - FWD2_WORKER_RESERVE) { p.mv = 1; p.wpx = per; p.wpw = waves; }
        }
    p.mh = (workers_env != 1 && p.mv == 1 && p.wpw == 4 && p.xw_half > 0) ? 1 : 0;
    p.me = (p.mh == 1 && workers_env != 2) ? FWD2_HALF_KSTEPS : 0;
    if (head != nullptr) p.nfw = ctc_head_nfw(d, head->C, head->U, p.wpx);
    const int kb = H / 128;
    p.fwd_flow = head != nullptr ? flow_fwd_kernel<true>(kb, pr, p.mv, p.mh, p.me) : flow_fwd_kernel<false>(kb, pr, p.mv, p.mh, p.me);
    p.bwd_flow = head != nullptr ? flow_bwd_kernel<true>(kb, pr) : flow_bwd_kernel<false>(kb, pr);
    p.fwd_lds = head != nullptr ? (size_t)2 * CF_FOLLOW_TEAM_FLOATS * sizeof(float) : 0;      // (ctc_follower's two teams)
    // two dG tiles, the dh reduction buffer, the stash, the down product's per-wave tiles (double-buffered), the partners' dG tiles
    p.bwd_lds = ((size_t)2 * 1024 + 2 * 8 * 256 + (FLOW2_WINDOW ? 2 : 1) * 8 * kb * 256 + (size_t)(flow2_q(kb, pr) - 1) * 1024) * sizeof(float);
    const size_t lds_workers = (size_t)2 * 2 * 2 * BK * LDS_LD * sizeof(float);         // two GEMM teams per workgroup
    if (p.bwd_lds < lds_workers) p.bwd_lds = lds_workers;
    if (p.bwd_lds < (size_t)2 * CF_LEAD_TEAM_FLOATS * sizeof(float)) p.bwd_lds = (size_t)2 * CF_LEAD_TEAM_FLOATS * sizeof(float);      // (ctc_leader's two teams)

    // in-kernel weight-gradient workers exist when some XCD carries no recurrence group; they take the LAST `share` % of the frames
    // (the first the recurrence finishes), the launches behind the kernel the rest
    const FlowGemmShare g = flow_gemm_share();
    const bool workers = g.pieces > 0 && g.percent > 0 && T >= 64 && groups < 8 && H % 128 == 0;
    // (split precision: the recurrence is ~1 us per step shorter, the f32 worker GEMMs are not)
    // (fused CTC head: the teams that run ctc_leader first join the weight-gradient work ~1 ms late -- 30 / 32 / 34 / 36 / 38 % ->
    //  12.43 / 12.47 / 12.38 / 12.30 / 12.56 ms per step on one box, the separate launches 12.67 - 12.88 there)
    // (round 6, reduced precisions WITH the head: the recurrence is a third shorter, the f32 worker products are not, and the leader
    //  teams still join ~1 ms late -- 16 / 20 / 24 / 28 % -> 8.20 / 8.32 / 8.54 / 9.12 ms per step in bf16x3 at 3x512 on one box (no
    //  workers: 8.53); round 5 ran it at 28 %: the "regression" of that mode against round 4's 8.60)
    const int share = g.set ? g.percent : (pr != 0 ? (head != nullptr ? g.percent / 2 - 1 : g.percent * 3 / 4) : g.percent);
    // dZ_0 = dG_0 . W_ih0^T by the bottom layer's groups (default since round 4: with the 2-D down product the kernel pays 0.2 ms
    // for it and the 0.61 ms GEMM + the mask launch behind the kernel go: 13.45 -> 13.36 ms per step; rounds 2-3, with the 32-way
    // exchange of down partials: a draw, off).  AMDSPEECH_FLOW_DZ0=0: the GEMM after the kernel.
    static const int dz0_in = runtime_switch("AMDSPEECH_FLOW_DZ0", 1);
    p.dz0_inkernel = dz0_in ? 1 : 0;
    p.w_dz0 = (p.dz0_inkernel || workers) ? 0 : 1;
    p.w_pieces = workers ? g.pieces : 0;
    static const int deal = runtime_switch("AMDSPEECH_FLOW_WORKER_DEAL", -1);      // -1: with the fused CTC head only; 0 / 1: never / always
    p.w_deal = workers && g.pieces <= 8 && (deal > 0 || (deal < 0 && head != nullptr));
    p.w_t0 = workers ? T - (int)((long)T * share / 100) : T;
    if (p.w_t0 < 2) p.w_t0 = 2;
    return p;
}

static LstmLayout lstm_layout(const LstmPlan& p) {
    const size_t T = p.d.T, B = p.d.B, H = p.d.H, L = p.d.L;
    const size_t tbh = T * B * H;
    LstmLayout o;
    size_t off = 0;
    auto take = [&](size_t n) { size_t r = off; off += (n + 63) / 64 * 64; return r; };
    // lstm_fwd_flow2's x-product workers: pre-multiplied gate tiles, [T][L][batch tiles][H/16][parts][256][4] (xw_half: and, behind
    // them in every frame, the half roles' [L][batch tiles][H/16][256][2] -- reserved by the shape, whatever the launch uses), written once per
    // launch and tagged with the launch's parity.  FIRST and time-major: frame t lives at the same address whatever T the
    // descriptor names (ops.LstmWorkspace.prefix lays ONE allocation out for every sequence length of a training run), so the
    // tags survive from one launch to the next with another T (AMDSPEECH_LSTM_SAME_WS)
    o.xwp = 0;
    if (p.xw_parts > 0) o.xwp = take(T * L * ((B + 15) / 16) * (H / 16) * (p.xw_parts * 1024 + p.xw_half * 512));
    o.wp = take(L * 2 * H * 4 * H);
    o.wq = take(L * 2 * H * 4 * H);
    o.z = take((L + 1) * tbh);
    o.hs = take(L * (T + 1) * B * H);
    o.cs = take(L * (T + 1) * B * H);
    o.gates = take(L * tbh * 4);
    o.dg = take(L * tbh * 4);
    o.dztop = take(tbh);
    o.dz0 = take(tbh);
    o.dc = take(L * 2 * B * H);
    // fragment-major ("packed") copies of the panels the NEXT diagonal consumes as MFMA A operands
    const size_t bp = (B + 15) / 16 * 16;
    o.xp0 = take(T * bp * H);          // layer-0 input, whole sequence
    o.xp = take(L * 2 * bp * H);       // layer l>=1 input, 2-slot ring (slot = diagonal parity)
    o.hp = take(L * 2 * bp * H);       // h_{t-1}, 2-slot ring
    o.dgp = take(L * 2 * bp * 4 * H);  // dG, 2-slot ring
    o.sync = take(64);                 // error word of the dataflow kernels, backward progress word, XCD tickets
    // full-history fragment-major panels of the dataflow kernels (every slot written once per sequence)
    o.xph = o.hph = o.dxh = o.prec = o.pdown = o.wopack = off;
    if (p.flow_shape) {
        o.xph = take((L + 1) * T * bp * H);    // layer l >= 1 input x_t  (slot [l][t]; [0][*] unused; [L][*]: the top layer's output for the fused CTC head)
        o.hph = take(L * (T + 1) * bp * H);    // h_{t-1}                  (slot [l][t]; [l][0] = initial state)
        // a SECOND set of the two (AMDSPEECH_LSTM_ARM_NEXT): a training cycle's forward calls alternate between the sets, and the
        // set the next call will use gets its sentinels beside THIS call's kernel -- not behind it, where the 330 MB fill met the
        // output layer and the log-softmax
        o.fwd_set = off - o.xph;
        take((L + 1) * T * bp * H);
        take(L * (T + 1) * bp * H);
        o.wopack = take((H / 16) * CF_NTC * 256);      // W_o as MFMA B fragments (fused CTC head)
        o.dxh = take(L * T * bp * H);          // dX_l[t]: gradient of layer l's output coming from layer l+1 (through memory)
        // lstm_bwd_flow2: partial-tile rings, [group][slots][H/16 consumers][H/16 producers][256 floats]
        const size_t slot = (size_t)L * (bp / 16) * (H / 16) * (H / 16) * 256;
        o.prec = take(2 * slot);               // rec partials: 2 slots
        o.pdown = take(4 * L * (bp / 16) * (H / 16) * (H / 128) * 256);   // down partials, summed per K slice: 4 slots of [H/16 consumers][H/128 K slices][256]
        // ... and, directly behind them (the kernel finds it there), the dG tiles the Q workgroups of a K slice show each other when
        // the recurrent product is cut both ways (flow2_q > 1): [group][2 slots][H/16][1024], tagged; zeroed with the rings
        take(L * (bp / 16) * 2 * (H / 16) * 1024);
    }
    // lstm_bwd_big (H = 1024), ONE layer at a time: the partial-tile rings of the two XCDs of every pair, [2 slots][batch tiles]
    // [2][32][32][256 floats], and the dG tiles that cross between them, [2 slots][batch tiles][64][1024]
    o.bigring = off;
    if (p.big_ring) o.bigring = take((size_t)2 * (bp / 16) * (2 * 32 * 32 * 256 + 64 * 1024));
    // precision = 2 at H = 1024 (gemm_bf16p.hip): bf16 copies of the batched products' operands + the split-K partial tiles
    o.bfs = off;
    if (p.bf16p_reserved) o.bfs = take(bf16p_scratch_floats(&p.d));
    o.total = off;
    return o;
}

// ------------------------------------------------------------------- one call, one direction
struct FwdCall {
    const amdspeech_lstm_desc* d; float* ws; const float* kernels; long kstride; const float* biases; long bstride;
    const int* lengths; const float* h0; const float* c0; const amdspeech_ctc_head* head;
    LstmPlan p; LstmLayout lo;      // (fwd_prologue)
};
struct BwdCall {
    const amdspeech_lstm_desc* d; float* ws; const float* kernels; long kstride; float* dkernels; float* dbiases; long bstride;
    const int* lengths; const amdspeech_ctc_head* head;
    LstmPlan p; LstmLayout lo;      // (bwd_prologue)
};
static DropCfg drop_cfg(const amdspeech_lstm_desc* d) { return DropCfg{d->keep_in, d->keep_out, d->seed, d->L}; }
// the layer-0 input dropout mask on dZ_0 (unless the kernel that formed dZ_0 applied it)
static int mask_dz0(hipStream_t s, const BwdCall& c) {
    if (c.d->keep_in < 1.0f) {
        const long n = (long)c.d->T * c.d->B * c.d->H;
        hipLaunchKernelGGL(apply_zmult_kernel, dim3(ceil_div(n, 256)), dim3(256), 0, s, c.ws + c.lo.dz0, n, drop_cfg(c.d), 0);
        AS_CHECK_LAUNCH();
    }
    return AMDSPEECH_OK;
}

// Every path: the fills a previous call on THIS workspace left on the side stream, the plan, the error word, the weight pack
static int fwd_prologue(hipStream_t s, FwdCall& c) {
    const amdspeech_lstm_desc* d = c.d;
    if (int rc = check_desc(d)) return rc;
    AS_CHECK_ARG(c.ws && c.kernels && c.biases && c.lengths, "lstm_fwd: null pointer");
    AS_CHECK_ARG(((uintptr_t)c.ws % 256) == 0, "lstm_fwd: workspace must be 256-byte aligned");
    if (int rc = flow_arm_settle(s, c.ws)) return rc;      // (see AMDSPEECH_LSTM_ARM_NEXT)
    if (int rc = flow_mark_prelaunch(s, c.ws, 0)) return rc;       // (until a dataflow launch says otherwise)
    c.p = lstm_plan(d, c.head);
    c.lo = lstm_layout(c.p);
    AS_CHECK_ARG(c.head == nullptr || c.p.fwd == Path::flow, "lstm_fwd_ctc: the fused CTC head needs the whole-sequence kernels (amdspeech_lstm_ctc_fusable)");
    prof_flops(0, 0.0, 0.0);
    AS_CHECK_HIP(hipMemsetAsync(c.ws + c.lo.sync, 0, 64, s));      // error word read by amdspeech_lstm_status (every path)
    const long wtotal = (long)d->L * 2 * d->H * 4 * d->H;
    if (c.p.fwd == Path::diag_bf3)
        hipLaunchKernelGGL(pack_fwd_bf3_kernel, dim3(ceil_div(wtotal, 256)), dim3(256), 0, s, c.kernels, c.kstride,
                           reinterpret_cast<unsigned short*>(c.ws + c.lo.wp), d->H, d->L);
    else
        hipLaunchKernelGGL(pack_fwd_kernel, dim3(ceil_div(wtotal, 256)), dim3(256), 0, s, c.kernels, c.kstride,
                           c.ws + c.lo.wp, d->H, d->L, c.p.uw, 0);
    AS_CHECK_LAUNCH();
    return AMDSPEECH_OK;
}
// The per-layer and per-diagonal paths: the initial state rows, the input dropout mask on Z_0, and the packed A panels -- the layer-0
// input of every frame (the per-diagonal kernels) and the initial h of every layer (slot of the first launch that reads it: diagonal
// l, or slot 0 for the per-layer kernels)
static int fwd_stage(hipStream_t s, const FwdCall& c) {
    const amdspeech_lstm_desc* d = c.d;
    const int T = d->T, B = d->B, H = d->H, L = d->L;
    float* ws = c.ws;
    const LstmLayout& lo = c.lo;
    const size_t bh = (size_t)B * H, bp = (size_t)(B + 15) / 16 * 16, n0 = (size_t)T * bh;
    for (int l = 0; l < L; ++l) {
        float* hs0 = ws + lo.hs + (size_t)l * (T + 1) * bh;
        float* cs0 = ws + lo.cs + (size_t)l * (T + 1) * bh;
        if (c.h0) AS_CHECK_HIP(hipMemcpyAsync(hs0, c.h0 + l * bh, bh * 4, hipMemcpyDeviceToDevice, s));
        else AS_CHECK_HIP(hipMemsetAsync(hs0, 0, bh * 4, s));
        if (c.c0) AS_CHECK_HIP(hipMemcpyAsync(cs0, c.c0 + l * bh, bh * 4, hipMemcpyDeviceToDevice, s));
        else AS_CHECK_HIP(hipMemsetAsync(cs0, 0, bh * 4, s));
    }
    if (d->keep_in < 1.0f) {
        hipLaunchKernelGGL(apply_zmult_kernel, dim3(ceil_div(n0, 256)), dim3(256), 0, s, ws + lo.z, (long)n0, drop_cfg(d), 0);
        AS_CHECK_LAUNCH();
    }
    if (c.p.fwd == Path::diag_bf3) {
        hipLaunchKernelGGL(pack_rows_bf3_kernel, dim3(ceil_div(n0, 256)), dim3(256), 0, s, ws + lo.z, bh,
                           reinterpret_cast<unsigned short*>(ws + lo.xp0), B, H, T);
        for (int l = 0; l < L; ++l)
            hipLaunchKernelGGL(pack_rows_bf3_kernel, dim3(ceil_div(bh, 256)), dim3(256), 0, s,
                               ws + lo.hs + (size_t)l * (T + 1) * bh, bh,
                               reinterpret_cast<unsigned short*>(ws + lo.hp + ((size_t)l * 2 + (l & 1)) * bp * H), B, H, 1);
    } else {
        const bool diag = c.p.fwd == Path::diag;
        if (diag)
            hipLaunchKernelGGL(pack_rows_kernel, dim3(ceil_div(n0, 256)), dim3(256), 0, s, ws + lo.z, bh, ws + lo.xp0, B, H, T);
        for (int l = 0; l < L; ++l)
            hipLaunchKernelGGL(pack_rows_kernel, dim3(ceil_div(bh, 256)), dim3(256), 0, s,
                               ws + lo.hs + (size_t)l * (T + 1) * bh, bh, ws + lo.hp + ((size_t)l * 2 + (diag ? (l & 1) : 0)) * bp * H,
                               B, H, 1);
    }
    AS_CHECK_LAUNCH();
    return AMDSPEECH_OK;
}

static int fwd_flow(hipStream_t s, const FwdCall& c) {
    const amdspeech_lstm_desc* d = c.d;
    const LstmPlan& p = c.p;
    const LstmLayout& lo = c.lo;
    float* ws = c.ws;
    const int T = d->T, B = d->B, H = d->H, L = d->L;
    const size_t bp = (size_t)(B + 15) / 16 * 16, bph = bp * H, bh = (size_t)B * H;
    const DropCfg dc = drop_cfg(d);
    unsigned* err = reinterpret_cast<unsigned*>(ws + lo.sync);
    // sentinel pre-fill of every slot the kernel will write (unless the previous forward call of the training cycle has
    // done it behind its own kernel: AMDSPEECH_LSTM_ARMED) ...
    const int set = (d->flags & AMDSPEECH_LSTM_ARMED) ? flow_clean_set(ws) : 0;
    if (!(d->flags & AMDSPEECH_LSTM_ARMED))
        if (int rc = flow_fill_fwd_panels(s, d, ws, lo, set)) return rc;
    float* const panels = ws + (size_t)set * lo.fwd_set;
    // ... then, in one launch each: the initial state (rows + packed slot 0 of every layer), error word and tickets; and
    // the layer-0 operand panels of all frames, the input dropout mask applied on the way
    hipLaunchKernelGGL(flow_fwd_prepare_kernel, dim3(ceil_div((long)L * bph, 256)), dim3(256), 0, s, c.h0, c.c0, ws + lo.hs, ws + lo.cs,
                       panels + lo.hph, err, T, B, H, L);
    hipLaunchKernelGGL(mask_pack_rows_kernel, dim3(ceil_div((long)T * bh / 4, 256)), dim3(256), 0, s, ws + lo.z, ws + lo.xp0, B, H, T,
                       dc, d->keep_in < 1.0f ? 1 : 0);
    AS_CHECK_LAUNCH();
    FlowArgs fa;
    fa.wp = ws + lo.wp; fa.bias = c.biases; fa.bias_stride = c.bstride;
    fa.z = ws + lo.z; fa.hs = ws + lo.hs; fa.cs = ws + lo.cs; fa.gates = ws + lo.gates; fa.lengths = c.lengths;
    fa.xp0 = ws + lo.xp0; fa.xph = panels + lo.xph; fa.hph = panels + lo.hph; fa.err = err;
    fa.T = T; fa.B = B; fa.H = H; fa.L = L; fa.drop = dc;
    fa.limit = p.limit;
    fa.trace = dev_trace_ptr(); fa.trace_layer = dev_knob("AMDSPEECH_TRACE_LAYER", L > 1 ? 1 : 0);      // (development builds only)
    fa.tickets = err + 16;
    fa.xwp = ws + lo.xwp; fa.xw_par = 0u; fa.w_wpx = p.wpx; fa.w_wpw = p.wpw;
    if (p.mv > 0)
        if (int rc = flow_xw_parity(s, ws, (d->flags & (AMDSPEECH_LSTM_ARMED | AMDSPEECH_LSTM_SAME_WS)) != 0,
                                    (((long)B * 4096 + H) * 64 + L) * 8 + p.mv * 2 + p.mh, fa.xwp,
                                    (size_t)L * (bp / 16) * (H / 16) * (p.mv * 1024 + p.mh * 512), T,
                                    &fa.xw_par)) return rc;
    fa.cf = CtcFlow{}; fa.cf_on = 0; fa.cf_nfw = 0;
    if (c.head != nullptr) {
        // the fused CTC head: extended targets and W_o's fragments first (both read by the follower workgroups of the launch)
        const amdspeech_ctc_head* head = c.head;
        AS_CHECK_ARG(p.nfw > 0, "lstm_fwd_ctc: this shape does not take the fused CTC head (amdspeech_lstm_ctc_fusable)");
        fa.cf = ctc_head_args(d, head, ws, lo, panels, p.nfw); fa.cf_on = 1; fa.cf_nfw = p.nfw;
        fa.cf.lengths = c.lengths; fa.cf.err = err; fa.cf.limit = fa.limit;
        if (int rc = ctc_prepare_targets(s, head->dense_labels, c.lengths, T, B, head->C, head->U, head->ctc_ws)) return rc;
        hipLaunchKernelGGL(ctc_pack_wo_kernel, dim3(ceil_div((H / 16) * CF_NTC * 64, 256)), dim3(256), 0, s, head->w_out, ws + lo.wopack, H, head->C);
        AS_CHECK_LAUNCH();
        AS_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(p.fwd_flow), hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.fwd_lds));
    }
    prof_begin(0, s);
    // ... and, in a training cycle, the backward call's panels go out beside the kernel (it leaves two XCDs idle)
    const bool arm = (d->flags & AMDSPEECH_LSTM_ARM_NEXT) != 0;
    if (arm)
        if (int rc = flow_arm_fork(s)) return rc;
    // (amdspeech_lstm_beside_forward; with x-product workers on the spare XCDs nothing is "idle": the next mini-batch's front end
    //  beside them cost the recurrence 0.1 - 0.2 ms and the step 0.06 - 0.13 -- the caller then places it beside the CTC stage)
    // (with the fused CTC head there is no CTC stage to place it beside: the remaining reserved workgroups' CUs take it again)
    if (int rc = flow_mark_prelaunch(s, ws, (p.mv > 0 && c.head == nullptr) ? 0 : 8 - L * p.nmt)) return rc;
    hipLaunchKernelGGL(p.fwd_flow, dim3(256), dim3(512), p.fwd_lds, s, fa);  // one workgroup per CU; each finds its group by XCC_ID
    prof_end(0, s, T + L - 1);
    prof_flops(0, (double)T * L * 2.0 * B * 2 * H * 4 * H, 0.0);
    AS_CHECK_LAUNCH();
    if (arm) {
        // beside the kernel (two XCDs and all of HBM idle): what lstm_bwd polls, its transposed weight pack, and the OTHER set
        // of forward panels for the next forward call of the same shape (rounds 2 - 3a re-filled this call's own set behind
        // the kernel: 330 MB beside the output layer and the log-softmax, +35 us on the critical path).  Nothing is joined
        // here: the next dataflow call on any stream waits for the side stream first (flow_arm_settle)
        // (The fills as ONE work-queue launch that really runs beside the forward kernel were built and measured in round 5 -- the
        //  forward kernel 4.46-4.51 -> 4.70-5.20 ms, the step 12.40-12.43 -> 12.59-12.73 ms: 550 MB of stores through the fabric the
        //  x-product workers and the CTC follower read through cost the recurrence more than the 0.1 ms these launches spend between
        //  the two recurrence kernels -- and removed in round 6.)
        if (int rc = flow_fill_bwd_panels(g_side, d, ws, lo, c.head != nullptr)) return rc;
        const long wtotal = (long)L * 2 * H * 4 * H;
        hipLaunchKernelGGL(pack_bwd_kernel, dim3(ceil_div(wtotal, 256)), dim3(256), 0, g_side, c.kernels, c.kstride, ws + lo.wq, H, L);
        AS_CHECK_LAUNCH();      // (the backward call's K^T pack: the weights do not change between the two halves of a cycle)
        if (int rc = flow_fill_fwd_panels(g_side, d, ws, lo, 1 - set)) return rc;
        if (int rc = flow_arm_publish(ws, 1 - set)) return rc;
    }
    return AMDSPEECH_OK;
}

// H = 1024 forward, layer by layer: one stack, or two side by side on the one-XCD groups (big1)
static int big_fwd_layers(hipStream_t s, int n, const FwdCall* st, bool big1) {
    const amdspeech_lstm_desc* d = st[0].d;
    const int T = d->T, B = d->B, H = d->H, L = d->L, nmt = ceil_div(B, 16);
    const size_t TB = (size_t)T * B, bp = (size_t)nmt * 16, bh = (size_t)B * H;
    if (big1) {
        static const hipError_t once = hipFuncSetAttribute(reinterpret_cast<const void*>(lstm_fwd_big1), hipFuncAttributeMaxDynamicSharedMemorySize, BIG1_LDS_BYTES);
        AS_CHECK_HIP(once);
    }
    BigFwd1Args b1;
    b1.n = n;
    for (int k = 0; k < n; ++k) {
        const FwdCall& q = st[k];
        unsigned* err = reinterpret_cast<unsigned*>(q.ws + q.lo.sync);
        BigFwdArgs& ba = b1.b[k];
        ba.wp = q.ws + q.lo.wp; ba.z = q.ws + q.lo.z; ba.hs = q.ws + q.lo.hs; ba.cs = q.ws + q.lo.cs; ba.gates = q.ws + q.lo.gates;
        ba.lengths = q.lengths;
        ba.err = err; ba.tickets = err + 16;
        ba.T = T; ba.B = B; ba.H = H; ba.L = L; ba.drop = drop_cfg(q.d);
        ba.limit = q.p.limit;
    }
    if (n == 1) b1.b[1] = b1.b[0];
    for (int l = 0; l < L; ++l) {
        for (int k = 0; k < n; ++k) {
            const FwdCall& q = st[k];
            float* ws = q.ws;
            const LstmLayout& lk = q.lo;
            // pre-activations of ALL frames: [T*B, H] . K_l[0:H, :] + b_l -> gates[l] (replaced frame by frame by the kernel)
            const float* z = ws + lk.z + (size_t)l * TB * H;
            float* g = ws + lk.gates + (size_t)l * TB * 4 * H;
            if (int rc = q.p.bf16p ? bf16p_xw(s, bf16p_bufs(q.d, ws + lk.bfs), (int)TB, H, z, q.kernels + l * q.kstride, g, q.biases + l * q.bstride)
                                   : gemm_batched(q.d, s, false, false, (int)TB, 4 * H, H, z, H, q.kernels + l * q.kstride, 4 * H, g, 4 * H,
                                                  q.biases + l * q.bstride, false)) return rc;
            // the h ring of this layer: slot 0 = the packed initial state with every word tagged 1, slot 1 = zeros (tag 0)
            float* ring = ws + lk.hp + (size_t)l * 2 * bp * H;
            AS_CHECK_HIP(hipMemsetAsync(ring, 0, 2 * bp * H * sizeof(float), s));
            hipLaunchKernelGGL(pack_rows_kernel, dim3(ceil_div(bh, 256)), dim3(256), 0, s,
                               ws + lk.hs + (size_t)l * (T + 1) * bh, bh, ring, B, H, 1);
            hipLaunchKernelGGL(tag_panel_kernel, dim3(ceil_div(bp * H, 256)), dim3(256), 0, s, ring, bp * H, 1u);
            AS_CHECK_HIP(hipMemsetAsync(b1.b[k].tickets, 0, 8 * sizeof(unsigned), s));
            b1.b[k].hring = ring; b1.b[k].layer = l;
        }
        if (n == 1) b1.b[1] = b1.b[0];
        prof_begin(0, s, l);
        if (big1) hipLaunchKernelGGL(lstm_fwd_big1, dim3(256), dim3(512), BIG1_LDS_BYTES, s, b1);
        else hipLaunchKernelGGL(st[0].p.fwd_big, dim3(256), dim3(512), 0, s, b1.b[0]);      // one workgroup per CU; each finds its place by XCC_ID
        prof_end(0, s, T * L, l);
    }
    AS_CHECK_LAUNCH();
    return AMDSPEECH_OK;
}
static int fwd_big(hipStream_t s, const FwdCall& c) {
    if (int rc = fwd_stage(s, c)) return rc;
    return big_fwd_layers(s, 1, &c, c.p.fwd == Path::big1);
}

static int fwd_diag(hipStream_t s, const FwdCall& c) {
    if (int rc = fwd_stage(s, c)) return rc;
    const amdspeech_lstm_desc* d = c.d;
    const int T = d->T, H = d->H, L = d->L;
    float* ws = c.ws;
    const LstmLayout& lo = c.lo;
    FwdArgs a;
    a.xp0 = ws + lo.xp0; a.xp = ws + lo.xp; a.hp = ws + lo.hp;
    a.wp = ws + lo.wp; a.bias = c.biases; a.bias_stride = c.bstride;
    a.z = ws + lo.z; a.hs = ws + lo.hs; a.cs = ws + lo.cs; a.gates = ws + lo.gates; a.lengths = c.lengths;
    a.T = T; a.B = d->B; a.H = H; a.L = L; a.drop = drop_cfg(d);
    a.hoist = 0; a.l0 = 0; a.mt0 = 0; a.dbg = 0;
    a.trace = dev_trace_ptr(); a.trace_d = a.trace ? dev_knob("AMDSPEECH_TRACE_D", T / 2) : -1;      // (development builds only)
    const dim3 grid = c.p.fwd == Path::diag_bf3 ? dim3(H / 8, L, ceil_div(c.p.nmt, 2)) : dim3(H / c.p.uw, L, c.p.nmt / c.p.fwd_mt);
    prof_begin(0, s);
    for (int dd = 0; dd < T + L - 1; ++dd) {
        a.d = dd;
        hipLaunchKernelGGL(c.p.fwd_diag, grid, dim3(8 * 64), 0, s, a);
    }
    prof_end(0, s, T + L - 1);
    AS_CHECK_LAUNCH();
    return AMDSPEECH_OK;
}

static int lstm_fwd(hipStream_t s, FwdCall c) {
    if (int rc = fwd_prologue(s, c)) return rc;
    switch (c.p.fwd) {
        case Path::flow: return fwd_flow(s, c);
        case Path::big: case Path::big1: return fwd_big(s, c);
        default: return fwd_diag(s, c);
    }
}

// Every path: the fills lstm_fwd left on the side stream, the plan, the weight pack K^T
static int bwd_prologue(hipStream_t s, BwdCall& c) {
    const amdspeech_lstm_desc* d = c.d;
    if (int rc = check_desc(d)) return rc;
    AS_CHECK_ARG(c.ws && c.kernels && c.dkernels && c.dbiases && c.lengths, "lstm_bwd: null pointer");
    if (int rc = flow_arm_settle(s, c.ws)) return rc;      // (see AMDSPEECH_LSTM_ARM_NEXT)
    if (int rc = flow_mark_postlaunch(s, c.ws, 0)) return rc;      // (until a dataflow launch says otherwise)
    c.p = lstm_plan(d, c.head);
    c.lo = lstm_layout(c.p);
    const long wtotal = (long)d->L * 2 * d->H * 4 * d->H;
    if (c.p.bwd == Path::diag_bf3)
        hipLaunchKernelGGL(pack_bwd_bf3_kernel, dim3(ceil_div(wtotal, 256)), dim3(256), 0, s, c.kernels, c.kstride,
                           reinterpret_cast<unsigned short*>(c.ws + c.lo.wq), d->H, d->L);
    else if (!(c.p.bwd == Path::flow && (d->flags & AMDSPEECH_LSTM_ARMED)))      // (armed: lstm_fwd packed K^T beside its kernel)
        hipLaunchKernelGGL(pack_bwd_kernel, dim3(ceil_div(wtotal, 256)), dim3(256), 0, s, c.kernels, c.kstride, c.ws + c.lo.wq, d->H, d->L);
    AS_CHECK_LAUNCH();
    AS_CHECK_ARG(c.head == nullptr || c.p.bwd == Path::flow, "lstm_bwd_ctc: the fused CTC head needs the whole-sequence kernels (amdspeech_lstm_ctc_fusable)");
    prof_flops(1, 0.0, 0.0);
    return AMDSPEECH_OK;
}
static BwdArgs bwd_args(const BwdCall& c) {
    const amdspeech_lstm_desc* d = c.d;
    float* ws = c.ws;
    const LstmLayout& lo = c.lo;
    BwdArgs a;
    a.hoist = 0; a.l0 = 0; a.mt0 = 0;
    a.wq = ws + lo.wq; a.cs = ws + lo.cs; a.gates = ws + lo.gates; a.dg = ws + lo.dg;
    a.dztop = ws + lo.dztop; a.dc = ws + lo.dc; a.lengths = c.lengths; a.dgp = ws + lo.dgp;
    a.T = d->T; a.B = d->B; a.H = d->H; a.L = d->L; a.drop = drop_cfg(d);
    return a;
}
// Time-independent weight gradients of the frames [ta, tb): dK_l += [Z_l ; Hprev_l]^T . dG_l, db_l += colsum(dG_l), and
// dZ_0 = dG_0 . K_0[0:H,:]^T of the frames [ta, dz_tb) (dZ_0 may cover more or fewer frames than the weight gradients)
static int weight_grads(hipStream_t s, const BwdCall& c, int ta, int tb, int dz_tb) {
    const amdspeech_lstm_desc* d = c.d;
    const LstmLayout& lo = c.lo;
    float* ws = c.ws;
    const int T = d->T, B = d->B, H = d->H, L = d->L;
    const size_t TB = (size_t)T * B, r0 = (size_t)ta * B;
    const int rows = (tb - ta) * B, dz_rows = (dz_tb - ta) * B;
    for (int l = 0; l < L; ++l) {
        const float* z = ws + lo.z + ((size_t)l * TB + r0) * H;
        const float* hp = ws + lo.hs + ((size_t)l * (T + 1) * B + r0) * H;      // slots 0..T-1 = h_{t-1}
        const float* dg = ws + lo.dg + ((size_t)l * TB + r0) * 4 * H;
        float* dk = c.dkernels + l * c.kstride;
        float* db = c.dbiases + l * c.bstride;
        if (c.p.bf16p && rows % 64 == 0 && rows >= 64) {
            // plain bf16 through operand copies: both halves of the layer's kernel gradient as ONE product, the bias gradient on
            // the transposing copy of dG
            if (int rc = bf16p_dk(s, bf16p_bufs(d, ws + lo.bfs), rows, H, z, hp, dg, dk, db)) return rc;
        } else if (d->precision != 0) {      // split precision: one launch per product, the bias gradient on its own
            if (int rc = gemm_reduced(d, s, true, false, H, 4 * H, rows, z, H, dg, 4 * H, dk, 4 * H, nullptr, true)) return rc;
            if (int rc = colsum_accumulate(s, dg, rows, 4 * H, 4 * H, db)) return rc;
            if (int rc = gemm_reduced(d, s, true, false, H, 4 * H, rows, hp, H, dg, 4 * H, dk + (size_t)H * 4 * H, 4 * H, nullptr, true)) return rc;
        } else {
            // the two products of a layer share dG_l, and 2 x 64 tiles x 2 K splits = one workgroup per CU: ONE launch per layer (all
            // 2 L in one launch put three waves on every SIMD and ran 30 % slower)
            const float* pa[2] = {z, hp}; const float* pb[2] = {dg, dg};
            float* pc[2] = {dk, dk + (size_t)H * 4 * H}; float* ps[2] = {db, nullptr};
            if (gemm_f32_tn_group_ok(H, 4 * H, rows, z, H, dg, 4 * H) && gemm_f32_tn_group_ok(H, 4 * H, rows, hp, H, dg, 4 * H)) {
                if (int rc = gemm_f32_tn_group(s, 2, H, 4 * H, rows, pa, H, pb, 4 * H, pc, 4 * H, ps, true)) return rc;
            } else {      // (operands the LDS-free kernel cannot address: the general GEMM, one product per launch)
                for (int i = 0; i < 2; ++i)
                    if (int rc = gemm_f32(s, true, false, H, 4 * H, rows, pa[i], H, pb[i], 4 * H, pc[i], 4 * H, nullptr, true, ps[i])) return rc;
            }
        }
    }
    if (dz_rows <= 0) return AMDSPEECH_OK;
    const float* dg0 = ws + lo.dg + r0 * 4 * H;
    float* dz0 = ws + lo.dz0 + r0 * H;
    if (c.p.bf16p && dz_rows >= 256) return bf16p_dx(s, bf16p_bufs(d, ws + lo.bfs), dz_rows, H, dg0, c.kernels, dz0);
    return gemm_batched(d, s, false, true, dz_rows, H, 4 * H, dg0, 4 * H, c.kernels, 4 * H, dz0, H, nullptr, false);
}
// dX_{l-1} [T*B, H] = dG_l [T*B, 4H] . K_l[0:H, :]^T, into the (by then dead) dztop buffer: hands a finished layer's gradient down
static int hand_down(hipStream_t s, const BwdCall& c, int l) {
    const amdspeech_lstm_desc* d = c.d;
    const int H = d->H;
    const size_t TB = (size_t)d->T * d->B;
    return gemm_batched(d, s, false, true, (int)TB, H, 4 * H, c.ws + c.lo.dg + (size_t)l * TB * 4 * H, 4 * H, c.kernels + l * c.kstride,
                        4 * H, c.ws + c.lo.dztop, H, nullptr, false);
}

static int bwd_flow(hipStream_t s, const BwdCall& c) {
    const amdspeech_lstm_desc* d = c.d;
    const LstmPlan& p = c.p;
    const LstmLayout& lo = c.lo;
    float* ws = c.ws;
    const int T = d->T, B = d->B, H = d->H, L = d->L;
    unsigned* err = reinterpret_cast<unsigned*>(ws + lo.sync);
    int* progress = reinterpret_cast<int*>(err) + 8;
    unsigned* tickets = err + 16;
    if (!(d->flags & AMDSPEECH_LSTM_ARMED))      // (else: lstm_fwd has prepared them beside its kernel)
        if (int rc = flow_fill_bwd_panels(s, d, ws, lo, c.head != nullptr)) return rc;
    AS_CHECK_HIP(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(progress), T, 8, s));
    AS_CHECK_HIP(hipMemsetAsync(tickets, 0, 16 * sizeof(unsigned), s));      // (+ the workers' eight item counters behind them)
#if FLOW2_CHECK_ORDER
    AS_CHECK_HIP(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(ws + lo.dg), (int)FLOW_SENTINEL, (size_t)L * T * B * 4 * H, s));
    AS_CHECK_HIP(hipMemsetAsync(ws + lo.pdown, 0, (lo.total - lo.pdown) * sizeof(float), s));
#endif
    FlowBwdArgs fb;
    fb.wq = ws + lo.wq; fb.cs = ws + lo.cs; fb.gates = ws + lo.gates; fb.dg = ws + lo.dg; fb.dztop = ws + lo.dztop;
    fb.prec = ws + lo.prec; fb.pdown = ws + lo.pdown;
    fb.nprog = p.nmt; fb.prog_slack = 0;
    fb.dxh = ws + lo.dxh; fb.tickets = tickets; fb.lengths = c.lengths; fb.err = err; fb.progress = progress;
    fb.T = T; fb.B = B; fb.H = H; fb.L = L; fb.drop = drop_cfg(d);
    fb.limit = p.limit;
    fb.trace = dev_trace_ptr();                                       // (development builds only; nullptr otherwise)
    fb.trace_layer = dev_knob("AMDSPEECH_TRACE_LAYER", L - 1);
    fb.cf = CtcFlow{}; fb.cf_on = 0;
    if (c.head != nullptr) {
        AS_CHECK_ARG(p.nfw > 0, "lstm_bwd_ctc: this shape does not take the fused CTC head (amdspeech_lstm_ctc_fusable)");
        fb.cf = ctc_head_args(d, c.head, ws, lo, nullptr, p.nfw); fb.cf_on = 1;
        fb.cf.lengths = c.lengths; fb.cf.err = err; fb.cf.limit = fb.limit;
    }
    AS_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(p.bwd_flow), hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.bwd_lds));
    fb.z = ws + lo.z; fb.hs = ws + lo.hs; fb.kernels = c.kernels; fb.dk = c.dkernels; fb.dbias = c.dbiases; fb.dz0 = ws + lo.dz0;
    fb.kstride = c.kstride; fb.bstride = c.bstride;
    fb.dz0_inkernel = p.dz0_inkernel;
    fb.w_dz0 = p.w_dz0;
    fb.w_mode = 0;
    fb.w_pieces = p.w_pieces;
    fb.w_counters = p.w_deal ? tickets + 8 : nullptr;
    fb.w_t0 = p.w_t0;
    prof_begin(1, s);
    hipLaunchKernelGGL(p.bwd_flow, dim3(256), dim3(512), p.bwd_lds, s, fb);      // one workgroup per CU; each finds its group by XCC_ID
    prof_end(1, s, T + L - 1);
    if (int rc = flow_mark_postlaunch(s, ws, 1 | (fb.dz0_inkernel ? 2 : 0))) return rc;      // (amdspeech_lstm_beside_tail)
    {   // algorithmic flops of this launch: L recurrent + (L - 1) down products (+ dZ_0 when the layer-0 groups form it) per
        // frame, and the weight-gradient products of the frames [w_t0, T) its worker workgroups take
        const double prod = 2.0 * B * 4 * H * H;
        const double wframes = fb.w_pieces > 0 ? (double)(T - fb.w_t0) : 0.0;
        prof_flops(1, (double)T * (2 * L - 1 + (fb.dz0_inkernel ? 1 : 0)) * prod,
                   wframes * (L * 2.0 * prod + (fb.w_dz0 ? prod : 0.0)));
    }
    AS_CHECK_LAUNCH();
    // what the workers did not take (dZ_0: nothing if the layer-0 groups formed it, else every frame)
    if (int rc = weight_grads(s, c, 0, p.w_pieces > 0 ? p.w_t0 : T, p.dz0_inkernel ? 0 : T)) return rc;
    return p.dz0_inkernel ? AMDSPEECH_OK : mask_dz0(s, c);
}

// H = 1024 backward in plain bf16 on the one-XCD groups (lstm_bwd_big1), layer by layer, top first: one stack, or two side by side
static int big1_bwd_layers(hipStream_t s, int n, const BwdCall* st) {
    const amdspeech_lstm_desc* d = st[0].d;
    const int T = d->T, B = d->B, H = d->H, L = d->L, nmt = ceil_div(B, 16);
    const size_t TB = (size_t)T * B;
    const size_t pring_floats = (size_t)2 * nmt * 2 * 32 * 32 * 256, xring_floats = (size_t)2 * nmt * 64 * 1024;
    BigBwd1Args b1;
    b1.n = n;
    for (int k = 0; k < n; ++k) {
        const BwdCall& q = st[k];
        const LstmLayout& lo = q.lo;
        unsigned* err = reinterpret_cast<unsigned*>(q.ws + lo.sync);
        BigBwdArgs& b2 = b1.b[k];
        b2.wq = q.ws + lo.wq; b2.cs = q.ws + lo.cs; b2.gates = q.ws + lo.gates; b2.dg = q.ws + lo.dg; b2.dup = q.ws + lo.dztop;
        b2.lengths = q.lengths; b2.pring = q.ws + lo.bigring; b2.xring = q.ws + lo.bigring + pring_floats; b2.err = err; b2.tickets = err + 16;
        b2.T = T; b2.B = B; b2.H = H; b2.L = L; b2.drop = drop_cfg(q.d);
        b2.limit = q.p.limit;
    }
    for (int l = L - 1; l >= 0; --l) {
        for (int k = 0; k < n; ++k) {
            AS_CHECK_HIP(hipMemsetAsync(b1.b[k].pring, 0, (pring_floats + xring_floats) * sizeof(float), s));
            AS_CHECK_HIP(hipMemsetAsync(b1.b[k].tickets, 0, 8 * sizeof(unsigned), s));
            b1.b[k].layer = l;
            const Bf16pBufs bufs = bf16p_bufs(st[k].d, st[k].ws + st[k].lo.bfs);
            b1.b[k].dgb = bufs.dgb; b1.b[k].dbias = st[k].dbiases + l * st[k].bstride;
        }
        if (n == 1) b1.b[1] = b1.b[0];
        prof_begin(1, s, L - 1 - l);
        hipLaunchKernelGGL(lstm_bwd_big1<BIG1_Q>, dim3(256), dim3(512), 0, s, b1);
        prof_end(1, s, T * L, L - 1 - l);
        for (int k = 0; k < n; ++k) {      // everything this layer owes, now (dZ_0 for the bottom layer)
            const BwdCall& q = st[k];
            float* ws = q.ws;
            if (int rc = bf16p_layer_bwd_copied(s, bf16p_bufs(q.d, ws + q.lo.bfs), (int)TB, H, ws + q.lo.z + (size_t)l * TB * H,
                                                ws + q.lo.hs + (size_t)l * (T + 1) * B * H, q.kernels + l * q.kstride,
                                                l > 0 ? ws + q.lo.dztop : ws + q.lo.dz0, q.dkernels + l * q.kstride)) return rc;
        }
    }
    AS_CHECK_LAUNCH();
    for (int k = 0; k < n; ++k)
        if (int rc = mask_dz0(s, st[k])) return rc;
    return AMDSPEECH_OK;
}

// H = 1024: one weight-stationary launch per layer (lstm_bwd_big), top first; after each, ONE GEMM hands the finished layer's
// gradient down (or, through the bf16 operand copies, everything this layer owes)
static int bwd_big(hipStream_t s, const BwdCall& c) {
    const amdspeech_lstm_desc* d = c.d;
    const LstmLayout& lo = c.lo;
    float* ws = c.ws;
    const int T = d->T, B = d->B, H = d->H, L = d->L, nmt = c.p.nmt;
    const size_t TB = (size_t)T * B;
    unsigned* err = reinterpret_cast<unsigned*>(ws + lo.sync);
    BigBwdArgs b2{};
    b2.wq = ws + lo.wq; b2.cs = ws + lo.cs; b2.gates = ws + lo.gates; b2.dg = ws + lo.dg; b2.dup = ws + lo.dztop; b2.lengths = c.lengths;
    const size_t pring_floats = (size_t)2 * nmt * 2 * 32 * 32 * 256, xring_floats = (size_t)2 * nmt * 64 * 1024;
    b2.pring = ws + lo.bigring; b2.xring = ws + lo.bigring + pring_floats; b2.err = err; b2.tickets = err + 16;
    b2.T = T; b2.B = B; b2.H = H; b2.L = L; b2.drop = drop_cfg(d);
    b2.limit = c.p.limit;
    for (int l = L - 1; l >= 0; --l) {
        AS_CHECK_HIP(hipMemsetAsync(ws + lo.bigring, 0, (pring_floats + xring_floats) * sizeof(float), s));
        AS_CHECK_HIP(hipMemsetAsync(b2.tickets, 0, 8 * sizeof(unsigned), s));
        b2.layer = l;
        prof_begin(1, s, L - 1 - l);
        hipLaunchKernelGGL(c.p.bwd_big, dim3(256), dim3(512), 0, s, b2);
        prof_end(1, s, T * L, L - 1 - l);
        if (c.p.bf16p) {      // plain bf16 through operand copies: everything this layer owes, now (dZ_0 for the bottom layer)
            if (int rc = bf16p_layer_bwd(s, bf16p_bufs(d, ws + lo.bfs), (int)TB, H, ws + lo.z + (size_t)l * TB * H,
                                         ws + lo.hs + (size_t)l * (T + 1) * B * H, ws + lo.dg + (size_t)l * TB * 4 * H, c.kernels + l * c.kstride,
                                         l > 0 ? ws + lo.dztop : ws + lo.dz0, c.dkernels + l * c.kstride, c.dbiases + l * c.bstride)) return rc;
        } else if (l > 0) {
            if (int rc = hand_down(s, c, l)) return rc;
        }
    }
    AS_CHECK_LAUNCH();
    if (!c.p.bf16p)
        if (int rc = weight_grads(s, c, 0, T, T)) return rc;
    return mask_dz0(s, c);
}

// layer by layer, top first: T launches of the recurrent product, then ONE GEMM hands the finished layer's gradient down
static int bwd_hoist(hipStream_t s, const BwdCall& c) {
    const amdspeech_lstm_desc* d = c.d;
    const int T = d->T, H = d->H, L = d->L;
    BwdArgs a = bwd_args(c);
    a.hoist = 1;
    const dim3 grid(H / 16, 1, c.p.nmt), block(8 * 64);
    prof_begin(1, s);
    for (int l = L - 1; l >= 0; --l) {
        a.l0 = l;
        for (int dd = 0; dd < T; ++dd) {
            a.d = dd;
            hipLaunchKernelGGL(c.p.bwd_diag, grid, block, 0, s, a);
        }
        if (l > 0)
            if (int rc = hand_down(s, c, l)) return rc;
    }
    prof_end(1, s, T * L);
    AS_CHECK_LAUNCH();
    if (int rc = weight_grads(s, c, 0, T, T)) return rc;
    return mask_dz0(s, c);
}

// One launch per diagonal; chunk c of the weight gradients covers frames [T*(nch-1-c)/nch, T*(nch-c)/nch): the chain walks time
// downwards, and every layer has finished frame t after diagonal (T-1-t) + (L-1)
static int bwd_diag(hipStream_t s, const BwdCall& c) {
    const amdspeech_lstm_desc* d = c.d;
    const int T = d->T, H = d->H, L = d->L, nch = DK_CHUNKS;
    BwdArgs a = bwd_args(c);
    // (CU-masked streams are "blocking" streams: against the legacy NULL stream every launch on them pays an
    // implicit cross-stream synchronisation -- measured 20 us per launch -- so the caller must be on a real stream)
    const int nside = (T >= 64 && s != nullptr && overlap_init() == 1) ? DK_SIDE : 0;
    hipStream_t chain_stream = s;
    if (nside > 0) {
        chain_stream = g_chain;
        AS_CHECK_HIP(hipEventRecord(g_ev_a, s));
        AS_CHECK_HIP(hipStreamWaitEvent(g_chain, g_ev_a, 0));
    }
    const dim3 grid(H / 16, L, c.p.nmt), block(8 * 64);
    prof_begin(1, chain_stream);
    int next_chunk = 0;
    for (int dd = 0; dd < T + L - 1; ++dd) {
        a.d = dd;
        hipLaunchKernelGGL(c.p.bwd_diag, grid, block, 0, chain_stream, a);
        if (next_chunk < nside) {
            const int ta = (int)((long)T * (nch - 1 - next_chunk) / nch), tb = (int)((long)T * (nch - next_chunk) / nch);
            if (dd == (T - 1 - ta) + (L - 1)) {
                AS_CHECK_HIP(hipEventRecord(g_ev_b, g_chain));
                AS_CHECK_HIP(hipStreamWaitEvent(g_gemm, g_ev_b, 0));
                if (int rc = weight_grads(g_gemm, c, ta, tb, tb)) return rc;
                ++next_chunk;
            }
        }
    }
    prof_end(1, chain_stream, T + L - 1);
    AS_CHECK_LAUNCH();
    if (nside > 0) {
        AS_CHECK_HIP(hipEventRecord(g_ev_a, g_chain));
        AS_CHECK_HIP(hipStreamWaitEvent(s, g_ev_a, 0));
        const int rest = (int)((long)T * (nch - nside) / nch);
        if (int rc = weight_grads(s, c, 0, rest, rest)) return rc;   // the rest, whole chip
        AS_CHECK_HIP(hipEventRecord(g_ev_c, g_gemm));
        AS_CHECK_HIP(hipStreamWaitEvent(s, g_ev_c, 0));
    } else {
        if (int rc = weight_grads(s, c, 0, T, T)) return rc;
    }
    return mask_dz0(s, c);
}

static int lstm_bwd(hipStream_t s, BwdCall c) {
    if (int rc = bwd_prologue(s, c)) return rc;
    switch (c.p.bwd) {
        case Path::flow: return bwd_flow(s, c);
        case Path::big1: return big1_bwd_layers(s, 1, &c);
        case Path::big: return bwd_big(s, c);
        case Path::hoist: return bwd_hoist(s, c);
        default: return bwd_diag(s, c);
    }
}

}  // namespace amdspeech

// ------------------------------------------------------------------- C ABI
using namespace amdspeech;

extern "C" int amdspeech_profile_enable(int on) {
    if (on && !g_prof_on) {
        for (int i = 0; i < 2; ++i)
            for (int k = 0; k < PROF_SEGS; ++k)
                for (int j = 0; j < 2; ++j) AS_CHECK_HIP(hipEventCreate(&g_prof_ev[i][k][j]));
    }
    if (!on && g_prof_on) {
        for (int i = 0; i < 2; ++i)
            for (int k = 0; k < PROF_SEGS; ++k)
                for (int j = 0; j < 2; ++j) (void)hipEventDestroy(g_prof_ev[i][k][j]);
        g_prof_valid[0] = g_prof_valid[1] = false;
    }
    g_prof_on = on != 0;
    return AMDSPEECH_OK;
}

extern "C" int amdspeech_profile_get(int which, float* elapsed_ms, int* time_steps) {
    AS_CHECK_ARG(which == 0 || which == 1, "profile_get: which must be 0 or 1");
    AS_CHECK_ARG(elapsed_ms && time_steps, "profile_get: null pointer");
    AS_CHECK_ARG(g_prof_on && g_prof_valid[which], "profile_get: nothing recorded (enable profiling first)");
    float total = 0.f;
    for (int k = 0; k < g_prof_nseg[which]; ++k) {
        float ms = 0.f;
        AS_CHECK_HIP(hipEventSynchronize(g_prof_ev[which][k][1]));
        AS_CHECK_HIP(hipEventElapsedTime(&ms, g_prof_ev[which][k][0], g_prof_ev[which][k][1]));
        total += ms;
    }
    *elapsed_ms = total;
    *time_steps = g_prof_launches[which];
    return AMDSPEECH_OK;
}

extern "C" int amdspeech_profile_get_flops(int which, double* recurrence_flops, double* other_flops) {
    AS_CHECK_ARG(which == 0 || which == 1, "profile_get_flops: which must be 0 or 1");
    AS_CHECK_ARG(recurrence_flops && other_flops, "profile_get_flops: null pointer");
    *recurrence_flops = g_prof_flops[which][0];
    *other_flops = g_prof_flops[which][1];
    return AMDSPEECH_OK;
}

// The bytes a workspace for sequences of UP TO d->T frames needs.  ops.LstmWorkspace.prefix lays one allocation out again for every
// shorter run length.  Of the regions lstm_plan reserves, two exist only below a sequence length (the 32-bit buffer resources of the
// whole-sequence kernels): the dataflow panels (flow_shape) and the x-product workers' tile history (xw_parts, 0 or 1 -- one size --
// and the half tiles in its frames, xw_half, which end at a shorter length); big_ring and bf16p_reserved do not depend on T.  A prefix
// just below a threshold can need MORE than the full length above it; with the set of regions fixed the size is monotone in T, so
// the maximum over T' <= T is taken at T or at the last T' of one of the sets.
extern "C" size_t amdspeech_lstm_workspace_bytes(const amdspeech_lstm_desc* d) {
    if (check_desc(d)) return 0;
    size_t need = lstm_layout(lstm_plan(d, nullptr)).total;
    amdspeech_lstm_desc q = *d;
    auto last_with = [&](auto pred) {      // the largest T' <= d->T with pred (true below a threshold, false above), or 0
        q.T = d->T;
        if (pred(lstm_plan(&q, nullptr))) return d->T;
        int lo = 0, hi = d->T;             // pred(lo) true (or lo == 0), pred(hi) false
        while (hi - lo > 1) { q.T = lo + (hi - lo) / 2; if (pred(lstm_plan(&q, nullptr))) lo = q.T; else hi = q.T; }
        return lo;
    };
    const int cand[3] = {last_with([](const LstmPlan& p) { return p.flow_shape; }),
                         last_with([](const LstmPlan& p) { return p.xw_parts > 0; }),
                         last_with([](const LstmPlan& p) { return p.xw_half > 0; })};
    for (int c : cand)
        if (c > 0 && c < d->T) { q.T = c; const size_t n = lstm_layout(lstm_plan(&q, nullptr)).total; if (n > need) need = n; }
    return need * sizeof(float);
}

extern "C" void* amdspeech_lstm_ws_ptr(const amdspeech_lstm_desc* d, void* ws, int which) {
    if (check_desc(d) || !ws) return nullptr;
    const LstmLayout lo = lstm_layout(lstm_plan(d, nullptr));
    float* w = static_cast<float*>(ws);
    const size_t tbh = (size_t)d->T * d->B * d->H;
    switch (which) {
        case AMDSPEECH_LSTM_WS_Z0: return w + lo.z;
        case AMDSPEECH_LSTM_WS_ZTOP: return w + lo.z + (size_t)d->L * tbh;
        case AMDSPEECH_LSTM_WS_DZTOP: return w + lo.dztop;
        case AMDSPEECH_LSTM_WS_DZ0: return w + lo.dz0;
        case AMDSPEECH_LSTM_WS_HFINAL: return w + lo.hs + (size_t)d->T * d->B * d->H;
        case AMDSPEECH_LSTM_WS_CFINAL: return w + lo.cs + (size_t)d->T * d->B * d->H;
        case AMDSPEECH_LSTM_WS_GATES: return w + lo.gates;
        default: set_error("lstm_ws_ptr: unknown region %d", which); return nullptr;
    }
}

// The multipliers the kernels above apply, as a tensor (tests feed them to the oracle's DropoutWrapper restatement): the SAME
// zmult() with the other mask switched off.
__global__ void export_zmult_kernel(float* out, long n, DropCfg c, int lp) {
    long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = zmult(c, lp, (uint32_t)i);
}
extern "C" int amdspeech_lstm_dropout_multipliers(void* stream, const amdspeech_lstm_desc* d, int which, int layer, float* out) {
    if (int rc = check_desc(d)) return rc;
    AS_CHECK_ARG(out != nullptr && (which == 0 || which == 1) && layer >= 0 && layer < d->L,
                 "lstm_dropout_multipliers: which must be 0 (input mask) or 1 (output mask), layer in [0, L)");
    DropCfg dc{which == 0 ? d->keep_in : 1.0f, which == 1 ? d->keep_out : 1.0f, d->seed, d->L};
    const long n = (long)d->T * d->B * d->H;
    hipLaunchKernelGGL(export_zmult_kernel, dim3(ceil_div(n, 256)), dim3(256), 0, static_cast<hipStream_t>(stream), out, n, dc,
                       which == 0 ? layer : layer + 1);
    AS_CHECK_LAUNCH();
    return AMDSPEECH_OK;
}

extern "C" int amdspeech_lstm_workspace_release(void* stream, void* ws) {
    AS_CHECK_ARG(ws != nullptr, "lstm_workspace_release: null workspace");
    return flow_arm_release(static_cast<hipStream_t>(stream), ws);
}

// (A CU-masked stream confined to the idle XCDs would be the obvious tool, and does not exist: hipExtStreamCreateWithCUMask
// applies ONE per-XCD CU pattern to all eight XCDs -- tools/cumask_probe.hip: a mask with only the bits of "XCDs 6 and 7" set
// enables all 256 CUs.  The caller's kernels are dealt to every XCD like any other; see amdspeech.h for what that means.)
extern "C" int amdspeech_lstm_beside_forward(void* stream, const void* ws) {
    AS_CHECK_ARG(ws != nullptr, "lstm_beside_forward: null workspace");
    std::lock_guard<std::mutex> lock(g_arm_mutex);
    auto it = g_arm.find(ws);
    if (it == g_arm.end() || it->second.idle_xcds <= 0 || it->second.pre == nullptr) return 0;
    AS_CHECK_HIP(hipStreamWaitEvent(static_cast<hipStream_t>(stream), it->second.pre, 0));
    return it->second.idle_xcds;
}

extern "C" int amdspeech_lstm_beside_tail(void* stream, const void* ws) {
    AS_CHECK_ARG(ws != nullptr, "lstm_beside_tail: null workspace");
    std::lock_guard<std::mutex> lock(g_arm_mutex);
    auto it = g_arm.find(ws);
    if (it == g_arm.end() || it->second.post_flags == 0 || it->second.post == nullptr) return 0;
    AS_CHECK_HIP(hipStreamWaitEvent(static_cast<hipStream_t>(stream), it->second.post, 0));
    return it->second.post_flags;
}

extern "C" int amdspeech_lstm_status(const amdspeech_lstm_desc* d, void* ws) {
    if (int rc = check_desc(d)) return rc;
    AS_CHECK_ARG(ws != nullptr, "lstm_status: null workspace");
    const LstmLayout lo = lstm_layout(lstm_plan(d, nullptr));
    unsigned err = 0;
    AS_CHECK_HIP(hipMemcpy(&err, static_cast<float*>(ws) + lo.sync, sizeof(err), hipMemcpyDeviceToHost));
    if (err != 0) {
        flow_xw_forget(ws);
        set_error("LSTM dataflow kernels: a bounded wait timed out (flags 0x%x: 1 = forward, 2 = backward -- the workgroups of "
                  "one launch were not all resident; 4 = a weight-gradient GEMM gave up waiting for the backward kernel, "
                  "8 = an x-product worker of the forward kernel gave up waiting for the layer below, "
                  "32 = the fused CTC head gave up waiting for the top layer, "
                  "e.g. under a tool that serialises kernels: set AMDSPEECH_FLOW_GEMM=0:0); results of this step are invalid", err);
        return AMDSPEECH_ETIMEOUT;
    }
    return AMDSPEECH_OK;
}

extern "C" int amdspeech_lstm_fwd(void* stream, const amdspeech_lstm_desc* d, void* ws, const float* kernels,
                                  long kernel_stride, const float* biases, long bias_stride,
                                  const int* lengths, const float* h0, const float* c0) {
    return lstm_fwd(static_cast<hipStream_t>(stream), FwdCall{d, static_cast<float*>(ws), kernels, kernel_stride, biases, bias_stride, lengths, h0, c0});
}

extern "C" int amdspeech_lstm_pair_fusable(const amdspeech_lstm_desc* d) {
    return d != nullptr && check_desc(d) == AMDSPEECH_OK && lstm_plan(d, nullptr).pair;
}
static bool pair_together(const amdspeech_lstm_desc* d_a, const void* ws_a, const amdspeech_lstm_desc* d_b, const void* ws_b) {
    return d_a->T == d_b->T && d_a->B == d_b->B && d_a->H == d_b->H && d_a->L == d_b->L && d_a->precision == d_b->precision &&
           ws_a != ws_b && amdspeech_lstm_pair_fusable(d_a) && amdspeech_lstm_pair_fusable(d_b);
}

extern "C" int amdspeech_lstm_fwd_pair(void* stream, const amdspeech_lstm_desc* d_a, void* ws_a, const float* kernels_a, const float* biases_a,
                                       const amdspeech_lstm_desc* d_b, void* ws_b, const float* kernels_b, const float* biases_b,
                                       long kernel_stride, long bias_stride, const int* lengths, const float* h0_a, const float* c0_a) {
    hipStream_t s = static_cast<hipStream_t>(stream);
    AS_CHECK_ARG(d_a && d_b, "lstm_fwd_pair: null descriptor");
    FwdCall two[2] = {{d_a, static_cast<float*>(ws_a), kernels_a, kernel_stride, biases_a, bias_stride, lengths, h0_a, c0_a},
                      {d_b, static_cast<float*>(ws_b), kernels_b, kernel_stride, biases_b, bias_stride, lengths, nullptr, nullptr}};
    if (!pair_together(d_a, ws_a, d_b, ws_b)) {
        if (int rc = lstm_fwd(s, two[0])) return rc;
        return lstm_fwd(s, two[1]);
    }
    for (FwdCall& c : two) {
        if (int rc = fwd_prologue(s, c)) return rc;
        if (int rc = fwd_stage(s, c)) return rc;
    }
    return big_fwd_layers(s, 2, two, true);
}

extern "C" int amdspeech_lstm_bwd_pair(void* stream, const amdspeech_lstm_desc* d_a, void* ws_a, const float* kernels_a, float* dkernels_a,
                                       float* dbiases_a, const amdspeech_lstm_desc* d_b, void* ws_b, const float* kernels_b, float* dkernels_b,
                                       float* dbiases_b, long kernel_stride, long bias_stride, const int* lengths) {
    hipStream_t s = static_cast<hipStream_t>(stream);
    AS_CHECK_ARG(d_a && d_b, "lstm_bwd_pair: null descriptor");
    BwdCall two[2] = {{d_a, static_cast<float*>(ws_a), kernels_a, kernel_stride, dkernels_a, dbiases_a, bias_stride, lengths},
                      {d_b, static_cast<float*>(ws_b), kernels_b, kernel_stride, dkernels_b, dbiases_b, bias_stride, lengths}};
    if (!pair_together(d_a, ws_a, d_b, ws_b) || lstm_plan(d_a, nullptr).bwd != Path::big1) {
        if (int rc = lstm_bwd(s, two[0])) return rc;
        return lstm_bwd(s, two[1]);
    }
    for (BwdCall& c : two)
        if (int rc = bwd_prologue(s, c)) return rc;
    return big1_bwd_layers(s, 2, two);
}

extern "C" int amdspeech_lstm_bwd(void* stream, const amdspeech_lstm_desc* d, void* ws, const float* kernels,
                                  long kernel_stride, float* dkernels, float* dbiases, long bias_stride,
                                  const int* lengths) {
    return lstm_bwd(static_cast<hipStream_t>(stream), BwdCall{d, static_cast<float*>(ws), kernels, kernel_stride, dkernels, dbiases, bias_stride, lengths});
}

/* The fused CTC head (ctc_flow.h) */
// The plan as plain numbers (amdspeech.h: amdspeech_lstm_plan_info): reads lstm_plan, decides nothing
extern "C" int amdspeech_lstm_plan(const amdspeech_lstm_desc* d, int C, int U, amdspeech_lstm_plan_info* out) {
    if (int rc = check_desc(d)) return rc;
    AS_CHECK_ARG(out != nullptr, "lstm_plan: null output");
    AS_CHECK_ARG((C > 0 && U > 0) || (C == 0 && U == 0), "lstm_plan: head C=%d U=%d (both 0: no head)", C, U);
    amdspeech_ctc_head h{};
    h.C = C; h.U = U;
    const LstmPlan p = lstm_plan(d, C > 0 ? &h : nullptr);
    const bool flow_bwd = p.bwd == Path::flow;
    static_assert((int)Path::flow == AMDSPEECH_LSTM_PATH_FLOW && (int)Path::big1 == AMDSPEECH_LSTM_PATH_BIG1 &&
                  (int)Path::big == AMDSPEECH_LSTM_PATH_BIG && (int)Path::hoist == AMDSPEECH_LSTM_PATH_HOIST &&
                  (int)Path::diag == AMDSPEECH_LSTM_PATH_DIAG && (int)Path::diag_bf3 == AMDSPEECH_LSTM_PATH_DIAG_BF3, "amdspeech.h");
    *out = amdspeech_lstm_plan_info{(int)p.fwd, (int)p.bwd, p.nmt, p.fwd == Path::flow ? d->H / 128 : 0, p.mv, p.wpx, p.uw, p.fwd_mt,
                                    p.pair ? 1 : 0, p.bf16p ? 1 : 0, p.bf16p_reserved ? 1 : 0, p.xw_parts, p.nfw, p.w_pieces,
                                    p.dz0_inkernel, flow_bwd ? flow2_q(d->H / 128, d->precision) : 0};
    return AMDSPEECH_OK;
}
// ... and what the 16 ints do not say of the forward dataflow launch: the x-product workers' share in HALF K blocks per recurrence wave
extern "C" int amdspeech_lstm_plan_xw_halves(const amdspeech_lstm_desc* d, int C, int U) {
    if (check_desc(d) != AMDSPEECH_OK) return -1;
    amdspeech_ctc_head h{};
    h.C = C; h.U = U;
    const LstmPlan p = lstm_plan(d, C > 0 ? &h : nullptr);
    return 2 * p.mv + p.mh;
}
// ... and the k-steps (of four) of the K block below the half roles' that those roles take as well (ME of lstm_fwd_flow2; 0: none)
extern "C" int amdspeech_lstm_plan_xw_ksteps(const amdspeech_lstm_desc* d, int C, int U) {
    if (check_desc(d) != AMDSPEECH_OK) return -1;
    amdspeech_ctc_head h{};
    h.C = C; h.U = U;
    const LstmPlan p = lstm_plan(d, C > 0 ? &h : nullptr);
    return p.me;
}
extern "C" int amdspeech_lstm_ctc_fusable(const amdspeech_lstm_desc* d, int C, int U) {
    if (check_desc(d) != AMDSPEECH_OK) return 0;
    amdspeech_ctc_head h{};
    h.C = C; h.U = U;
    return lstm_plan(d, &h).nfw > 0 ? 1 : 0;
}
static int check_head(const amdspeech_ctc_head* h, bool bwd) {
    AS_CHECK_ARG(h != nullptr, "lstm_*_ctc: null head");
    AS_CHECK_ARG(h->w_out && h->b_out && h->logits && h->dense_labels && h->loss && h->ctc_ws && (!bwd || h->dlogits),
                 "lstm_*_ctc: null pointer in the head");
    AS_CHECK_ARG(((uintptr_t)h->w_out % 16) == 0 && ((uintptr_t)h->ctc_ws % 256) == 0, "lstm_*_ctc: W_o must be 16-byte, the CTC workspace 256-byte aligned");
    return AMDSPEECH_OK;
}
extern "C" int amdspeech_lstm_fwd_ctc(void* stream, const amdspeech_lstm_desc* d, void* ws, const float* kernels,
                                      long kernel_stride, const float* biases, long bias_stride, const int* lengths,
                                      const float* h0, const float* c0, const amdspeech_ctc_head* head) {
    if (int rc = check_head(head, false)) return rc;
    return lstm_fwd(static_cast<hipStream_t>(stream), FwdCall{d, static_cast<float*>(ws), kernels, kernel_stride, biases, bias_stride, lengths, h0, c0, head});
}
extern "C" int amdspeech_lstm_bwd_ctc(void* stream, const amdspeech_lstm_desc* d, void* ws, const float* kernels,
                                      long kernel_stride, float* dkernels, float* dbiases, long bias_stride,
                                      const int* lengths, const amdspeech_ctc_head* head) {
    if (int rc = check_head(head, true)) return rc;
    return lstm_bwd(static_cast<hipStream_t>(stream), BwdCall{d, static_cast<float*>(ws), kernels, kernel_stride, dkernels, dbiases, bias_stride, lengths, head});
}

// ------------------------------------------- layer-wise bidirectional stacks: their kernels, then their host driver (lstm_bidir.h)
namespace amdspeech {
#include "lstm_layer.h"
#include "lstm_layer_bf3.h"
#include "lstm_bidir.h"
}  // namespace amdspeech
