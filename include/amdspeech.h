/*
 * amdspeech.h -- C ABI of libamdspeech.so (gfx950 / MI355X).
 *
 * Drop-in boundary for the acoustic-model hot path of domerin0/rnn-speech
 * (audio -> MFCC/fbank -> Linear -> stacked LSTM -> Linear -> CTC loss+grad ->
 * clip + Adam).  The reference has no FFI seam of its own: every one of these
 * ops is a TensorFlow-1.x / librosa call issued from
 * /root/reference/models/AcousticModel.py and /root/reference/util/audioprocessor.py.
 * Each entry point below names the reference call site it replaces; the Python
 * class surface above it (models.AcousticModel, util.audioprocessor.AudioProcessor)
 * is kept verbatim by rnn-speech_amd/ and binds these symbols through ctypes
 * (see INTEGRATION.md for the stub).
 *
 * Conventions
 *   - plain C, no torch types; every tensor is a caller-owned DEVICE pointer,
 *     contiguous, float32 unless stated (int32 for lengths / labels);
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream); all
 *     work is enqueued on it, nothing synchronises the device;
 *   - workspaces are caller-allocated, sized by the *_workspace_bytes queries;
 *   - return value: 0 = ok, negative = AMDSPEECH_E*; amdspeech_last_error()
 *     returns the message of the calling thread's last failure;
 *   - time-major activations [T, B, *]; the LSTM kernel of layer l is the TF
 *     BasicLSTMCell matrix K_l [2H, 4H] (rows: x then h; column blocks i|j|f|o),
 *     bias_l [4H]; forget_bias 1.0 is added at run time, never stored.
 */
#ifndef AMDSPEECH_H
#define AMDSPEECH_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AMDSPEECH_OK 0
#define AMDSPEECH_EINVAL (-1)   /* bad argument (shape, alignment, null pointer) */
#define AMDSPEECH_EHIP (-2)     /* a HIP runtime call failed */
#define AMDSPEECH_EUNSUPPORTED (-3)
#define AMDSPEECH_ETIMEOUT (-4) /* amdspeech_lstm_status: a bounded wait of a whole-sequence kernel gave up -- that mini-batch's results are
                                   invalid and it can be repeated (AMDSPEECH_LSTM_PER_DIAGONAL); every other error there is a device fault */

int amdspeech_version(void);
const char* amdspeech_last_error(void);
/* Number of compute units of the current device (sanity / grid sizing). */
int amdspeech_device_cu_count(void);

/* ---------------------------------------------------------------- Linear ----
 * y[M,N] = x[M,K] . w[K,N] + b[N]           (b may be NULL)
 * Replaces the per-frame tf.matmul(...) + bias lists of the input and output
 * layers, models/AcousticModel.py:247-250 and :308-309.                      */
int amdspeech_linear_fwd(void* stream, const float* x, const float* w, const float* b,
                         float* y, int M, int K, int N);
/* Backward of the above (what tf.gradients emits for :247-250/:308-309):
 *   dx[M,K]  = dy . w^T              (dx may be NULL: skipped)
 *   dw[K,N] += x^T . dy              (ACCUMULATES -- the reference's gradient
 *   db[N]   += column sums of dy      accumulators, :391-401)                */
int amdspeech_linear_bwd(void* stream, const float* x, const float* w, const float* dy,
                         float* dx, float* dw, float* db, int M, int K, int N);

/* General f32 MFMA GEMM used by the two calls above (exposed for tests/bench):
 * C[M,N] (+)= op(A)[M,K] . op(B)[K,N] (+ bias[N]).  transX != 0 means the
 * operand is stored transposed (A as [K,M], B as [N,K]); ld* are row strides
 * in elements.  accumulate != 0 adds into C.                                 */
int amdspeech_gemm_f32(void* stream, int transA, int transB, int M, int N, int K,
                       const float* A, int lda, const float* B, int ldb,
                       float* C, int ldc, const float* bias, int accumulate);

/* The same product in split precision ("bf16x3", the arithmetic of amdspeech_lstm_desc.precision = 1): every f32 operand value
 * is used as a bf16 pair hi = rne(x), lo = rne(x - hi) and every product as hi.hi + hi.lo + lo.hi on the bf16 MFMA with f32
 * accumulation (~16 significant bits per operand); operands and result stay float32 in memory.  Used by lstm_fwd / lstm_bwd
 * for their batched products at H = 1024 in that mode; exposed for tests and benchmarks.  A and B must be 16-byte aligned. */
int amdspeech_gemm_bf16x3(void* stream, int transA, int transB, int M, int N, int K,
                          const float* A, int lda, const float* B, int ldb,
                          float* C, int ldc, const float* bias, int accumulate);

/* ... and with PLAIN bf16 operands (round 4; the arithmetic of amdspeech_lstm_desc.precision = 2, BASELINE configs[4]'s "bf16
 * MFMA"): every f32 operand value is rounded to ONE bf16 (nearest even, 8 significant bits), every product is one bf16 MFMA,
 * accumulation and the result are float32; operands stay float32 in memory (the master copies).  Same contract otherwise.   */
int amdspeech_gemm_bf16(void* stream, int transA, int transB, int M, int N, int K,
                        const float* A, int lda, const float* B, int ldb,
                        float* C, int ldc, const float* bias, int accumulate);

/* Which kernel one of the three products above takes for a shape, and its launch geometry, as plain numbers: a READ-ONLY view of
 * the plan every product is launched from (one function plans for both).  Nothing is launched and no device is touched; the
 * pointers are inspected for null and alignment only, never dereferenced.  Arguments are checked as the call checks them, with
 * the call's own message.
 *   precision  0 amdspeech_gemm_f32, 1 amdspeech_gemm_bf16x3, 2 amdspeech_gemm_bf16 (as amdspeech_lstm_desc.precision): 1 and 2 report
 *              family BF3 or, where that kernel's addressing does not fit, what the f32 ladder takes instead
 *   colsum     != 0: with the fused column sums of B (amdspeech_linear_bwd's weight-gradient product)
 *   count      1: the single product; 2 .. AMDSPEECH_GEMM_GROUP_MAX: amdspeech_gemm_f32_tn_group (A, B, C: problem 0's operands)
 * The struct:
 *   family     AMDSPEECH_GEMM_* below
 *   variant    the kernel's template arguments as the launch switches on them: SKINNY_N NT (1 .. 6); SKINNY_K KT * 2 + transB
 *              (KT 3 or 5); SKINNY_TN FULL * 8 + RT; TN_DIRECT the number of problems; KC_DIRECT transB; LDS A_KC * 2 + B_KC
 *              (A_KC = !transA, B_KC = transB); BF3 single * 4 + A_KC * 2 + B_KC; BF16P (amdspeech_gemm_bf16_packed_plan only)
 *              A_KC * 2 + B_KC: which operand copy converts in place (KC) and which transposes
 *   splits, k_chunk   K ranges and their length (SKINNY_TN: row chunks, those that start past K add nothing);  atomic: the result
 *              leaves through f32 atomics;  zero_fill: a fill launch precedes;  grid: workgroups of the main launch
 *   tiles_m, tiles_n  output tiles (SKINNY_*: row blocks / 64-column slices)
 *   map        workgroup -> tile: AMDSPEECH_GEMM_MAP_* below;  bm, bn: the block of MAP_XCD_BLOCKS;  col_slices: SKINNY_K's slices of N
 *   a_vec, b_vec      16-byte loads on that operand (0: the scalar loads of the LDS kernel)                                     */
enum { AMDSPEECH_GEMM_SKINNY_N = 0, AMDSPEECH_GEMM_SKINNY_K = 1, AMDSPEECH_GEMM_SKINNY_TN = 2, AMDSPEECH_GEMM_TN_DIRECT = 3,
       AMDSPEECH_GEMM_KC_DIRECT = 4, AMDSPEECH_GEMM_LDS = 5, AMDSPEECH_GEMM_BF3 = 6, AMDSPEECH_GEMM_BF16P = 7 };
enum { AMDSPEECH_GEMM_MAP_LINEAR = 0, AMDSPEECH_GEMM_MAP_XCD = 1, AMDSPEECH_GEMM_MAP_XCD_BLOCKS = 2, AMDSPEECH_GEMM_MAP_KC_BAND = 3 };
enum { AMDSPEECH_GEMM_GROUP_MAX = 10 };
typedef struct amdspeech_gemm_plan_info {
    int family, variant, splits, k_chunk, atomic, zero_fill, grid, tiles_m, tiles_n, map, bm, bn, col_slices, a_vec, b_vec;
} amdspeech_gemm_plan_info;
int amdspeech_gemm_plan(int precision, int transA, int transB, int M, int N, int K,
                        const void* A, int lda, const void* B, int ldb, const void* C, int ldc,
                        const void* bias, int accumulate, int colsum, int count,
                        amdspeech_gemm_plan_info* out);

/* Exposed for tests / bench: `count` (1 .. AMDSPEECH_GEMM_GROUP_MAX) products C_i[M,N] (+)= A_i^T . B_i of ONE shape in one launch (the
 * weight gradients of an LSTM backward pass); A_i [K][M], B_i [K][N], rows 16-byte aligned.  A, B, C, colsum: HOST arrays of `count`
 * device pointers; colsum (or single entries of it) may be NULL, else colsum_i[N] += column sums of B_i.  A shape or an operand
 * the kernel does not take is AMDSPEECH_EINVAL (no other kernel is tried).  Bytes between the width and the stride of an
 * operand row are read and must be readable (their values reach no result).                                                     */
int amdspeech_gemm_f32_tn_group(void* stream, int count, int M, int N, int K, const float* const* A, int lda,
                                const float* const* B, int ldb, float* const* C, int ldc, float* const* colsum, int accumulate);
/* out[c] += sum over rows of x[r * ld + c]: the bias gradients of the reduced-precision path. */
int amdspeech_colsum_accumulate(void* stream, const float* x, int rows, int cols, int ld, float* out);
/* ... the same product through bf16 COPIES of the operands (round 5; what lstm_fwd / lstm_bwd run at H = 1024 with precision = 2):
 * each operand is copied once as bf16 with the contraction index contiguous (a 64 x 64 transpose where it is not), a 256 x 256 x 64
 * kernel streams the copies into LDS with global_load_lds, split K goes through f32 partial tiles (no atomics).  Same values
 * per operand as amdspeech_gemm_bf16 (round to nearest even), another summation order.  `scratch`: 256-byte aligned,
 * amdspeech_gemm_bf16_packed_scratch_bytes(...) bytes -- 0 from that query means the shape is not taken (K % 64, transposed
 * operands in multiples of 64, M, N >= 256): call amdspeech_gemm_bf16 instead.                                              */
size_t amdspeech_gemm_bf16_packed_scratch_bytes(int transA, int transB, int M, int N, int K, int lda, int ldb);
int amdspeech_gemm_bf16_packed(void* stream, int transA, int transB, int M, int N, int K,
                               const float* A, int lda, const float* B, int ldb,
                               float* C, int ldc, const float* bias, int accumulate, void* scratch, size_t scratch_bytes);
/* The plan of that call's product kernel, READ-ONLY as amdspeech_gemm_plan (one function plans for launch and query): family
 * AMDSPEECH_GEMM_BF16P, variant A_KC * 2 + B_KC, tiles_m x tiles_n tiles of 256 x 256, `splits` K ranges of k_chunk = 32 * (k tiles
 * per split) whose partial tiles one reduce launch adds up (atomic = zero_fill = 0), grid = tiles * splits.  A shape the call does
 * not take (scratch bytes 0) is AMDSPEECH_EINVAL with the call's message.  amdspeech_gemm_plan itself knows no precision 3.    */
int amdspeech_gemm_bf16_packed_plan(int transA, int transB, int M, int N, int K, int lda, int ldb, amdspeech_gemm_plan_info* out);
/* Exposed for tests: the operand copies of that path, as lstm_fwd / lstm_bwd share them between products.  bf16 values are
 * unsigned shorts, rounded to nearest even; src and dst 16-byte aligned, ld a multiple of 4.
 *   amdspeech_bf16_copy, transpose == 0: dst[rows][cols] = bf16(src[rows][ld]) -- dense (ldd == cols), cols a multiple of 8, no
 *     colsum, no plain;  transpose != 0: dst[cols][ldd] = bf16(src)^T in 64 x 64 tiles (rows, cols multiples of 64, ldd a multiple
 *     of 8, >= rows; columns rows .. ldd of dst are not written), colsum[c] += sum over r of src[r][c] (f32 atomics) when given,
 *     plain[rows][cols] = bf16(src) (dense, 16-byte aligned) when given: the row-major copy from the same read.
 *   amdspeech_bf16_transpose: dst[cols][ldd] = src[rows][cols]^T, src dense bf16; the same tiles and conditions.                 */
int amdspeech_bf16_copy(void* stream, const float* src, long ld, long rows, int cols, int transpose, unsigned short* dst, long ldd,
                        float* colsum, unsigned short* plain);
int amdspeech_bf16_transpose(void* stream, const unsigned short* src, long rows, int cols, unsigned short* dst, long ldd);

/* ----------------------------------------------------------- batch norm ----
 * Optional normalisation of the input-layer output, models/AcousticModel.py:253-259
 * (`batch_normalization : True` in config.ini; off by default): moments over the
 * BATCH axis only, per (t, feature); y = (x - mean) / sqrt(var + eps), biased variance,
 * eps = 1e-3 in the reference, no scale/offset, no running statistics.
 *   x, y, xhat: [T,B,H] (y may alias x; xhat, the saved normalised value, may be NULL
 *   when no backward follows); inv_std: [T,H].  Backward: dx from dy, xhat, inv_std. */
int amdspeech_batchnorm_fwd(void* stream, const float* x, float* y, float* xhat,
                            float* inv_std, int T, int B, int H, float eps);
int amdspeech_batchnorm_bwd(void* stream, const float* dy, const float* xhat,
                            const float* inv_std, float* dx, int T, int B, int H);

/* The same normalisation under data parallelism: tf.nn.moments then spans the GLOBAL batch (n_total = B * world), so every
 * sum over the batch axis is "local sum -> amdspeech_allreduce_sum_f32 -> finish".  Forward: batchnorm_sum(x, NULL) ->
 * all-reduce [T,H] -> batchnorm_sum(x, global_sum) (sum of squared deviations from the global mean) -> all-reduce ->
 * batchnorm_apply.  Backward: batchnorm_bwd_sums ([2][T,H]: sum dy, sum dy*xhat) -> all-reduce -> batchnorm_bwd_apply.  */
int amdspeech_batchnorm_sum(void* stream, const float* x, const float* global_sum, int n_total, float* out,
                            int T, int B, int H);
int amdspeech_batchnorm_apply(void* stream, const float* x, const float* global_sum, const float* global_sq,
                              int n_total, float eps, float* y, float* xhat, float* inv_std, int T, int B, int H);
int amdspeech_batchnorm_bwd_sums(void* stream, const float* dy, const float* xhat, float* sums, int T, int B, int H);
int amdspeech_batchnorm_bwd_apply(void* stream, const float* dy, const float* xhat, const float* inv_std,
                                  const float* global_sums, int n_total, float* dx, int T, int B, int H);

/* ------------------------------------------------------------ LSTM stack ----
 * Replaces tf.contrib.rnn.BasicLSTMCell + DropoutWrapper + MultiRNNCell +
 * tf.nn.dynamic_rnn(sequence_length, initial_state, time_major=True),
 * models/AcousticModel.py:223-237 and :266-298, and its BPTT gradient.
 *
 * Parameters live wherever the caller keeps them: layer l's kernel is at
 * kernels + l*kernel_stride, its bias at biases + l*bias_stride (elements).
 *
 * Workspace (one allocation, reused by fwd and bwd of the same step) holds the
 * repacked weights, the inter-layer activations Z_l [L+1][T][B][H], the state
 * history h/c [L][T+1][B][H], the activated gates [L][T][B][4H] and the gate
 * gradients.  Z_0 (the input of layer 0 = output of the input Linear) and
 * dZ_L (gradient arriving at the top) are views INTO that workspace obtained
 * with amdspeech_lstm_ws_ptr so the neighbouring GEMMs write them in place.  */
typedef struct amdspeech_lstm_desc {
    int T, B, H, L;
    float keep_in, keep_out;   /* DropoutWrapper keep probabilities (1 = off) */
    uint64_t seed;             /* dropout stream; the same seed in fwd and bwd */
    int precision;             /* 0: exact f32 MFMA (default, what the reference computes);
                                  1: "bf16x3" split products hi.hi + hi.lo + lo.hi with f32
                                     accumulation (~16 significant bits per operand), needs H % 32 == 0;
                                  2: "bf16" (round 4) every operand of the recurrent AND the batched products rounded to
                                     ONE bf16 (8 significant bits), one MFMA per product, f32 accumulation; gates, cell
                                     state, gradients, master weights stay f32.  Measured against float64 over ~1000 frames
                                     (DESIGN.md 4.2d): logits 1.3-2.3e-3 of max (outside north_star's 1e-3), CTC loss
                                     7e-5, gradients 3-5e-3 -- an opt-in throughput mode, never the default.  Shapes outside
                                     the dataflow / per-layer kernels run their RECURRENT products in bf16x3 (a superset
                                     in accuracy); the batched products (weight gradients, dZ_0) are single bf16 there too.
                                  The layer-wise bidirectional entry points (amdspeech_lstm_bidir_*) take 0 and 1 only */
    int flags;                 /* 0, or AMDSPEECH_LSTM_* bits below (training cycles on ONE workspace and shape) */
} amdspeech_lstm_desc;

/* The whole-sequence kernels poll hand-off panels inside the workspace that have to hold a sentinel when the launch starts
 * (forward: 330 MB at the benchmark shape; backward: the dX panels and two rings).  In a training cycle
 * lstm_fwd -> lstm_bwd -> lstm_fwd ... on ONE workspace and shape the fills come off the critical path:
 *   ARM_NEXT  (lstm_fwd) prepare, beside the forward kernel (it leaves two XCDs idle) and on a side stream of the library: the
 *             backward call's panels, its transposed weight pack (from `kernels`, which must not change before that call),
 *             and the forward panels of the NEXT forward call -- the workspace holds two sets of them and the calls of a
 *             cycle alternate (until round 3 this call's own set was re-filled behind its kernel, i.e. beside the caller's
 *             output layer).  The next lstm_fwd / lstm_bwd call makes its stream wait for that side stream first.
 *   ARMED     (lstm_bwd) the lstm_fwd before it, on this workspace and with the same T/B/H/L/precision, had ARM_NEXT;
 *             (lstm_fwd) the previous lstm_fwd on this workspace had ARM_NEXT and the same T/B/H/L/precision.
 *             The call then skips its fill.  Passing ARMED when that is not true makes the kernels read stale panels (their
 *             bounded waits then end in AMDSPEECH_ETIMEOUT at the next lstm_status).
 *   SAME_WS   (lstm_fwd, round 5) the previous lstm_fwd on this workspace ran with the same B / H / L / precision -- T may differ --
 *             and nothing but lstm calls has written to the workspace since; ARMED implies it.  What it protects (H = 512, exact
 *             f32, at least one XCD without a recurrence group): the forward kernel's x-product workers hand the recurrence
 *             groups pre-multiplied gate tiles through a write-once history that every workspace layout keeps at offset 0,
 *             frame-major (frame t at the same address whatever T), and whose words carry the LAUNCH's parity in their least
 *             significant mantissa bit.  A call with ARMED / SAME_WS flips the parity the previous launch left and, when it runs
 *             more frames than that launch, re-tags only the frames beyond it; any other lstm_fwd zeroes the frames it will use
 *             first (0.8 GB at 3 x 512, B = 32, T = 1001: once per training run).  A launch that ended in a time-out
 *             invalidates the parity (lstm_status forgets it).
 * The bits are ignored by the paths that have no such panels.
 * Surviving a time-out (round 5).  The whole-sequence kernels need every workgroup of a launch resident at once; when another
 * process holds CUs (or a tool serialises kernels) their bounded waits give up, the launch ends within its limit and
 * amdspeech_lstm_status reports it: that mini-batch's results are invalid.  The caller then discards its gradient contribution
 * and repeats lstm_fwd AND lstm_bwd of the mini-batch with
 *   PER_DIAGONAL    this call runs on the launch-per-diagonal kernels (what AMDSPEECH_FLOW=0 and, at 1024 units, AMDSPEECH_BIG=0
 *                   select for a whole process: no kernel with a bounded wait; same workspace, same layout, same results) -- rnn-speech_amd/acoustic_model.py does exactly that, logs once
 *                   and goes on (the reference's loop never loses a step: models/AcousticModel.py:887-939);
 *   INJECT_TIMEOUT  testing only: the persistent kernels of THIS call (whole-sequence, or per layer at 1024 units) give up on
 *                   their first unsatisfied wait (limit 0); passed to lstm_bwd it does the same to THAT call's persistent kernels
 *                   (lstm_bwd_flow2 with its workers and the CTC leader, lstm_bwd_big / _big1).                                 */
enum { AMDSPEECH_LSTM_ARMED = 1, AMDSPEECH_LSTM_ARM_NEXT = 2, AMDSPEECH_LSTM_SAME_WS = 4, AMDSPEECH_LSTM_PER_DIAGONAL = 8,
       AMDSPEECH_LSTM_INJECT_TIMEOUT = 16 };

enum {
    AMDSPEECH_LSTM_WS_Z0 = 0,      /* float [T][B][H]  in : layer-0 input          */
    AMDSPEECH_LSTM_WS_ZTOP = 1,    /* float [T][B][H]  out: top layer output       */
    AMDSPEECH_LSTM_WS_DZTOP = 2,   /* float [T][B][H]  in : dLoss/d(top output)    */
    AMDSPEECH_LSTM_WS_DZ0 = 3,     /* float [T][B][H]  out: dLoss/d(layer-0 input) */
    AMDSPEECH_LSTM_WS_HFINAL = 4,  /* float [L][B][H] slices of the h history at T */
    AMDSPEECH_LSTM_WS_CFINAL = 5,
    AMDSPEECH_LSTM_WS_GATES = 6    /* float [L][T][B][4][H] out: the activated gates i, j, f, o of every frame (the BPTT stash) */
};
size_t amdspeech_lstm_workspace_bytes(const amdspeech_lstm_desc* d);
/* Pointer of a named region inside `ws` (NULL on bad arguments). For
 * HFINAL/CFINAL the region of layer l is at ptr + l*(T+1)*B*H floats.        */
void* amdspeech_lstm_ws_ptr(const amdspeech_lstm_desc* d, void* ws, int which);

/* Ownership.  The library never allocates or frees a workspace and keeps no pointer into one EXCEPT between a call with
 * ARM_NEXT and the next lstm call on the same workspace (its side stream is then still writing the hand-off panels).  Before
 * freeing (or re-purposing) a workspace that has seen ARM_NEXT, call amdspeech_lstm_workspace_release: it makes `stream` wait
 * for that work and forgets the workspace; memory freed in stream order after it is safe.  All other state of the library is
 * per process and device, created on first use and never tied to caller memory: constant tables of the front end (twiddles,
 * mel filters, DCT; keyed by mode / sample rate / n_mfcc / device), one side stream + two events, the CU-masked streams of
 * the launch-per-diagonal overlap, the profiling events, and the calling thread's error text.  lstm_fwd / lstm_bwd are not
 * re-entrant on ONE workspace; calls on different workspaces are independent.                                               */
int amdspeech_lstm_workspace_release(void* stream, void* ws);

/* Work BESIDE the forward recurrence.  The whole-sequence forward kernel (H <= 512, L * ceil(B/16) <= 8 groups) keeps one
 * recurrence group per XCD (group g on XCD g) and leaves the other 8 - L * ceil(B/16) XCDs without work for the length of the
 * sequence (two of eight, ~5 ms, at 3 x 512 / batch 32).  This orders `stream` behind the point just in front of the last
 * amdspeech_lstm_fwd launch on `ws` and returns the number of idle XCDs (> 0); 0 (nothing ordered) when that call was not such
 * a launch, or (round 5: H = 512, exact f32) when the kernel's own x-product workers occupy the spare XCDs -- place the work
 * elsewhere (beside the CTC stage) -- unless the call carried the fused CTC head (amdspeech_lstm_fwd_ctc): there is no CTC stage
 * then, and the workgroups the kernel keeps in reserve on the spare XCDs are reported again.  What may follow on `stream`:
 *   - kernels small enough to share a CU with a recurrence workgroup (<= 32 VGPRs, no LDS to speak of: fills, packs): they run
 *     at once, everywhere;
 *   - WORK-QUEUE kernels (each workgroup pulls items from a counter until it is empty): the dispatcher deals the workgroups of
 *     any kernel round-robin to all eight XCDs, and those dealt to an XCD full of recurrence workgroups wait there until the
 *     recurrence ends -- but the ones on the idle XCDs drain the queue meanwhile, and the late ones find it empty.  The WORK is
 *     done beside the recurrence; the kernel (and whatever follows it in `stream`) completes when the recurrence does.  The
 *     front end's frame kernel is built this way (amdspeech_frontend_*).
 * A kernel with a fixed item per workgroup gains nothing here: 6/8 of it runs after the recurrence.  A stream confined to the
 * idle XCDs cannot be had (CU masks are one pattern for all XCDs).  Independent, short-lived work only: the dataflow kernels
 * spin on their siblings, so work that itself waited for them would deadlock.  Call it after amdspeech_lstm_fwd has returned. */
int amdspeech_lstm_beside_forward(void* stream, const void* ws);

/* Work BESIDE the weight-gradient launches that follow the backward recurrence (round 5).  amdspeech_lstm_bwd's whole-sequence
 * kernel is followed, on the caller's stream, by the products its in-kernel workers left over (three launches of 0.66 ms at the
 * headline shape, one 256-thread workgroup per CU: every CU has room for more waves).  This orders `stream` behind the point
 * BETWEEN that kernel and those launches and returns 1 | 2: 1 = ordered, 2 = DZ0 is complete at that point (the bottom layer's
 * groups formed it inside the kernel); 0 = the last amdspeech_lstm_bwd on `ws` was not such a launch (nothing ordered).  Short
 * products that only need the backward kernel's results -- dW_o / db_o from ZTOP and dlogits, dW_i / db_i from DZ0 -- then run
 * beside the first of the launches instead of behind the last.  The caller joins `stream` before it reads their results. */
int amdspeech_lstm_beside_tail(void* stream, const void* ws);

/* Forward over the whole stack.  h0/c0: [L][B][H] initial state or NULL (zeros)
 * -- the reference's persistent state Variables, :266-275.  lengths: int32 [B]
 * (device).  Frames t >= lengths[b] emit 0 and copy the state through.       */
int amdspeech_lstm_fwd(void* stream, const amdspeech_lstm_desc* d, void* ws,
                       const float* kernels, long kernel_stride,
                       const float* biases, long bias_stride,
                       const int* lengths, const float* h0, const float* c0);
/* TWO stacks of the same shape over the same batch, each in its own workspace -- the two directions of a bidirectional model
 * (BASELINE configs[4]; the caller hands stack B the time-reversed input in its Z0).  Same results as amdspeech_lstm_fwd(a ...) followed
 * by amdspeech_lstm_fwd(b ..., h0 = c0 = NULL).  Where the forward kernel can place a batch tile's recurrence group on ONE XCD (1024 wide
 * in plain bf16, ceil(B/16) <= 4: lstm_fwd_big1) every layer of the two stacks runs in ONE launch, stack A on XCDs 0 - 3 and stack B on
 * XCDs 4 - 7; everywhere else this IS the two calls -- amdspeech_lstm_pair_fusable(d) says which (1 = side by side), so that a caller
 * that keeps state between calls (the ARMED / ARM_NEXT cycle of the whole-sequence kernels) goes on making them itself.  (Two
 * amdspeech_lstm_fwd calls on two streams do not overlap: see lstm_big_fwd.h.)                                                      */
int amdspeech_lstm_pair_fusable(const amdspeech_lstm_desc* d);
int amdspeech_lstm_fwd_pair(void* stream, const amdspeech_lstm_desc* d_a, void* ws_a, const float* kernels_a, const float* biases_a,
                            const amdspeech_lstm_desc* d_b, void* ws_b, const float* kernels_b, const float* biases_b,
                            long kernel_stride, long bias_stride, const int* lengths, const float* h0_a, const float* c0_a);
/* ... and their backward passes (dZTOP of either workspace filled by the caller): the results of two amdspeech_lstm_bwd calls; side by
 * side under the same conditions (lstm_bwd_big1: W_hh^T as bf16 in the registers of one XCD per batch tile).                          */
int amdspeech_lstm_bwd_pair(void* stream, const amdspeech_lstm_desc* d_a, void* ws_a, const float* kernels_a, float* dkernels_a, float* dbiases_a,
                            const amdspeech_lstm_desc* d_b, void* ws_b, const float* kernels_b, float* dkernels_b, float* dbiases_b,
                            long kernel_stride, long bias_stride, const int* lengths);
/* Synchronous health check of the last forward/backward on `ws` (device sync + 4-byte
 * read): AMDSPEECH_ETIMEOUT if a bounded dataflow wait of the persistent kernels timed out (recoverable: repeat the mini-batch),
 * AMDSPEECH_EHIP if the read itself failed (a sticky device fault: not recoverable). */
int amdspeech_lstm_status(const amdspeech_lstm_desc* d, void* ws);
/* BPTT.  Reads DZTOP, the forward history in ws; writes DZ0 and ACCUMULATES
 * dK_l into dkernels + l*kernel_stride and db_l into dbiases + l*bias_stride. */
int amdspeech_lstm_bwd(void* stream, const amdspeech_lstm_desc* d, void* ws,
                       const float* kernels, long kernel_stride,
                       float* dkernels, float* dbiases, long bias_stride,
                       const int* lengths);

/* The CTC head INSIDE the whole-sequence kernels (round 5).  Between the two recurrence launches of a training step the reference
 * runs its output layer and tf.nn.ctc_loss (models/AcousticModel.py:241-247, :356-357); as separate launches (output Linear,
 * log-softmax, alpha / beta, gradient, dlogits . W_o^T) that is a serial 0.5 ms of a 12.7 ms step.  With a head attached
 *   lstm_fwd_ctc  also forms logits [T][B][C] = Z_top . W_o + b_o, their log-softmax and the alpha recursion, 16 frames behind the
 *                 top layer, on workgroups of the XCDs that carry no recurrence group: logits, loss [B] (= -log p(l|x), 0 for an
 *                 utterance whose targets do not fit its frames) and, in `ctc_ws`, log p / alpha / the extended targets are
 *                 complete when the launch is;
 *   lstm_bwd_ctc  runs beta, the posterior, dlogits [T][B][C] and dZ_top = dlogits . W_o^T ahead of the top layer's recurrence
 *                 groups on the workgroups that later form the weight gradients, then BPTT as lstm_bwd.  DZTOP is produced
 *                 inside the launch: the caller writes nothing there; dW_o / db_o (from ZTOP and dlogits) stay the caller's.
 * Same semantics as amdspeech_ctc_loss_fwd_bwd on the same logits: the loss is bit-identical (same device code), dlogits
 * equal to ~1e-7 (the order LDS atomics meet in).  A head on lstm_fwd_ctc obliges the caller to run lstm_bwd_ctc (not lstm_bwd)
 * for that mini-batch, or no backward pass at all.  amdspeech_lstm_ctc_fusable says whether a descriptor takes the head: the
 * whole-sequence kernels (H % 128 == 0, H <= 512, at least one XCD without a recurrence group), C one of 16, 32, 48, 64 and 80,
 * 2 U + 1 <= 384 extended states, B within two utterances per follower team; AMDSPEECH_FLOW_CTC=0 switches it off.  `ctc_ws`:
 * amdspeech_ctc_workspace_bytes(T, B, C, U) bytes, 256-byte aligned, the same T as the descriptor's.                          */
typedef struct amdspeech_ctc_head {
    const float* w_out;        /* [H][C] output Linear weight (16-byte aligned) */
    const float* b_out;        /* [C] */
    float* logits;             /* out (fwd): [T][B][C] */
    const int* dense_labels;   /* [B][U] 0-padded targets (the reference's labels_ph) */
    float* loss;               /* out (fwd): [B] */
    float* dlogits;            /* out (bwd): [T][B][C]; may be NULL for lstm_fwd_ctc */
    void* ctc_ws;
    int C, U;
} amdspeech_ctc_head;
int amdspeech_lstm_ctc_fusable(const amdspeech_lstm_desc* d, int C, int U);
int amdspeech_lstm_fwd_ctc(void* stream, const amdspeech_lstm_desc* d, void* ws,
                           const float* kernels, long kernel_stride, const float* biases, long bias_stride,
                           const int* lengths, const float* h0, const float* c0, const amdspeech_ctc_head* head);
int amdspeech_lstm_bwd_ctc(void* stream, const amdspeech_lstm_desc* d, void* ws,
                           const float* kernels, long kernel_stride, float* dkernels, float* dbiases, long bias_stride,
                           const int* lengths, const amdspeech_ctc_head* head);

/* The inverted-dropout multipliers (mask / keep_prob, [T][B][H]) that lstm_fwd / lstm_bwd with this descriptor apply:
 * which = 0 the INPUT mask of `layer`, which = 1 its OUTPUT mask -- tf.contrib.rnn.DropoutWrapper(cell, input_keep_prob,
 * output_keep_prob), models/AcousticModel.py:227-233: independent masks per layer and side, scale 1/keep, the state is never
 * masked.  The masks are a pure function of (seed, layer, side, element index t*B*H + b*H + h); the export exists so that a
 * checker can run the reference's graph with the very masks the kernels used.                                            */
int amdspeech_lstm_dropout_multipliers(void* stream, const amdspeech_lstm_desc* d, int which, int layer, float* out);

/* The kernel path lstm_fwd / lstm_bwd take for a descriptor, as plain numbers: a READ-ONLY view of the plan both calls make from
 * (T, B, H, L, precision, flags) and the fused head's (C, U) -- C = U = 0: no head.  Nothing is launched and nothing is decided
 * here; the query exists so that a test (or a log line) can name the kernel a shape runs instead of inferring it.  The whole-sequence
 * and per-layer paths ask the device for its CU count: without an MI355X every shape answers DIAG / DIAG_BF3.
 *   fwd_path, bwd_path  AMDSPEECH_LSTM_PATH_* below
 *   nmt                 16-row batch tiles;  kb = H / 128 on the FLOW path (K blocks per wave and half), else 0
 *   uw                  units per workgroup of the forward weight pack (launch-per-diagonal: 4 or 8; 16 elsewhere)
 *   fwd_mt              16-row M tiles per workgroup of lstm_fwd_step (1 or 2)
 *   mv, wpx             FLOW forward: x-product workers (K blocks per recurrence wave, 0: none), their workgroups per spare XCD
 *   xw_parts            ... the tile history the workspace reserves for them (0 or 1)
 *   nfw                 the fused CTC head's followers per spare XCD (0: no head, or the shape does not take it)
 *   pair                two stacks of this shape run side by side (amdspeech_lstm_pair_fusable)
 *   bf16p               the batched products of this call go through bf16 operand copies (precision 2, H = 1024, T * B a multiple
 *                       of 64 and >= 256);  bf16p_reserved: the workspace holds room for them whatever T
 *   w_pieces            FLOW backward: chunks of in-kernel weight-gradient work (0: none);  dz0_inkernel: dZ_0 formed in the kernel
 *   flow2_q             FLOW backward: workgroups that share a K slice of the recurrent product (1, 2 or 4; 0 off that path)    */
enum { AMDSPEECH_LSTM_PATH_FLOW = 0, AMDSPEECH_LSTM_PATH_BIG1 = 1, AMDSPEECH_LSTM_PATH_BIG = 2, AMDSPEECH_LSTM_PATH_HOIST = 3,
       AMDSPEECH_LSTM_PATH_DIAG = 4, AMDSPEECH_LSTM_PATH_DIAG_BF3 = 5 };
typedef struct amdspeech_lstm_plan_info {
    int fwd_path, bwd_path, nmt, kb, mv, wpx, uw, fwd_mt, pair, bf16p, bf16p_reserved, xw_parts, nfw, w_pieces, dz0_inkernel, flow2_q;
} amdspeech_lstm_plan_info;
int amdspeech_lstm_plan(const amdspeech_lstm_desc* d, int C, int U, amdspeech_lstm_plan_info* out);
/* The x-product workers' share of the FLOW forward launch in HALF K blocks per recurrence wave, which the 16 ints above cannot say
 * (`mv` counts whole blocks): 0 none, 2 one block (full roles on the spare XCDs), 3 a block and a half (half roles on waves 4-7 of
 * the worker workgroups too: gates f and o of a second K block -- exact f32, H = 512, one full role per SIMD fits); -1: bad
 * descriptor.  Read-only like amdspeech_lstm_plan.  The environment switch AMDSPEECH_FLOW_FWD_WORKERS (read once per process)
 * picks among the kernels a shape can take: 0 = no workers, 1 = full roles only, 2 or unset = half roles where they fit
 * (2: exactly round 6's; unset: the half roles extended by k-steps, below).                                                  */
int amdspeech_lstm_plan_xw_halves(const amdspeech_lstm_desc* d, int C, int U);
/* ... and how many of the four k-steps of the K block BELOW the half roles' block those roles take as well, for their two N tiles
 * (gates f, o) and into the same tile -- more K, not more N: the frame of the workers' tile history and the workspace size do not
 * change; the recurrence waves multiply those two tiles of that block for the other k-steps only.  0: none (no half roles, or
 * AMDSPEECH_FLOW_FWD_WORKERS=2); -1: bad descriptor.  amdspeech_lstm_plan_xw_halves keeps counting whole half blocks (3).        */
int amdspeech_lstm_plan_xw_ksteps(const amdspeech_lstm_desc* d, int C, int U);

/* ------------------------------------------------ layer-wise bidirectional stacks ----
 * tf.contrib.rnn.stack_bidirectional_dynamic_rnn (torch.nn.LSTM(bidirectional=True, num_layers=L)): L layers, each a forward and
 * a backward BasicLSTMCell (+ DropoutWrapper), where layer l+1 of BOTH directions reads the concatenation [h_fw_l ; h_bw_l].
 * (amdspeech_lstm_fwd_pair is the other, "top-joined" form: two independent stacks joined only in front of the output layer.)
 * Semantics:
 *   - layer 0 of both directions reads Z_0 [T][B][H] (the input Linear's output, region Z0);
 *   - for l >= 1 the forward cell reads [h_fw_{l-1} ; h_bw_{l-1}] [T][B][2H], fw half first (TF's concat(outputs, 2)); the
 *     backward cell reads tf.reverse_sequence of that concatenation, each row reversed within its own length; h_bw is stored
 *     in forward time;
 *   - cell kernels keep the TF BasicLSTMCell layout [input_depth + H][4H] (rows: x then h; column blocks i|j|f|o), bias [4H],
 *     forget_bias 1.0 added at run time: (2H, 4H) at layer 0, (3H, 4H) above.  `kernels` / `biases` are HOST arrays of 2L
 *     device pointers, the forward cells' layers 0..L-1 first, then the backward cells'.  The output layer reads
 *     [h_fw_top ; h_bw_top] (regions YTOP_FW / YTOP_BW);
 *   - dropout (desc keep_in / keep_out / seed): DropoutWrapper on each direction's cell -- its own input mask over its whole
 *     input (2H wide above layer 0) and its own output mask, in the cell's own (step) order: element s*B*W + b*W + k of step s.
 *     The forward cells draw from `seed`, the backward cells from seed ^ 0x5bd1e995; amdspeech_lstm_bidir_dropout_multipliers
 *     exports them (dir 0 / 1, which 0 = input mask [T][B][W], 1 = output mask [T][B][H]);
 *   - frames t >= len_b emit 0 and copy the state through; h0 / c0 ([L][B][H] or NULL) initialise the FORWARD cells, the backward
 *     cells start from zero; HFINAL / CFINAL are the forward cells' final state, layer l at ptr + l * layer_stride floats.
 * Precision 0 (exact f32; H a multiple of 16 up to 1024) or 1 (bf16x3: the recurrent product on the bf16 MFMA and the batched
 * products through the bf16x3 GEMM; H a multiple of 32 whose H and 4H rows of W_hh split over at most 8 waves in 32 x 1, 2, 4,
 * 8 or 16 rows: 32 ... 256, 320, 512, 768, 1024 and others -- workspace_bytes returns 0 for the rest); precision 2 (plain bf16):
 * AMDSPEECH_EUNSUPPORTED.  Per layer: the pack of both
 * directions' inputs, x . W_ih for all frames (one GEMM per direction), then ONE persistent launch for both directions' recurrence
 * (amdspeech_lstm_bidir_path = 2; 1 = one persistent launch per direction; 0 = one launch per frame: AMDSPEECH_BIDIR_PERSISTENT=0,
 * or flags & AMDSPEECH_LSTM_PER_DIAGONAL -- the repeat of a mini-batch whose persistent launch timed out).  Its bounded waits
 * end in AMDSPEECH_ETIMEOUT at amdspeech_lstm_bidir_status; AMDSPEECH_LSTM_INJECT_TIMEOUT (tests) gives up at the first
 * unsatisfied wait.  bwd reads DYTOP_FW / DYTOP_BW (forward time, filled by the caller), writes DZ0 and ACCUMULATES the cells'
 * kernel and bias gradients.                                                                                                  */
enum {
    AMDSPEECH_BIDIR_WS_Z0 = 0, AMDSPEECH_BIDIR_WS_YTOP_FW = 1, AMDSPEECH_BIDIR_WS_YTOP_BW = 2, AMDSPEECH_BIDIR_WS_DYTOP_FW = 3,
    AMDSPEECH_BIDIR_WS_DYTOP_BW = 4, AMDSPEECH_BIDIR_WS_DZ0 = 5, AMDSPEECH_BIDIR_WS_HFINAL = 6, AMDSPEECH_BIDIR_WS_CFINAL = 7
};
size_t amdspeech_lstm_bidir_workspace_bytes(const amdspeech_lstm_desc* d);
void* amdspeech_lstm_bidir_ws_ptr(const amdspeech_lstm_desc* d, void* ws, int which);
long amdspeech_lstm_bidir_layer_stride(const amdspeech_lstm_desc* d);
int amdspeech_lstm_bidir_path(const amdspeech_lstm_desc* d);      /* = the plan's `path`, below */
/* What amdspeech_lstm_bidir_fwd / _bwd on this descriptor launch for the recurrence -- each call plans once and launches from this;
 * read-only: nothing is launched, no pointer is dereferenced, d->flags & AMDSPEECH_LSTM_PER_DIAGONAL is honoured.  Errors: those
 * of the other entry points for the descriptor (AMDSPEECH_EUNSUPPORTED: precision 2, a hidden size the kernels do not take),
 * AMDSPEECH_EINVAL for a null `out`.
 *   path                2 / 1 / 0 as above;  cus: the device's compute units the path was planned for (0: no device, path 0)
 *   fwd_* / bwd_*       the recurrence kernel of the forward / backward call:
 *     kpw               bf16x3: K blocks of 32 per wave, the instantiation lstm_layer_{fwd,bwd}_bf3<KPW> (0 at precision 0)
 *     waves             waves of 64 threads per workgroup (precision 0: 8)
 *     groups            bf16x3: groups of 4 (forward) / 2 (backward) 16-row batch tiles per block of hidden units (precision 0: 1)
 *     wgs               workgroups PER DIRECTION: a path-2 and a per-frame launch have 2 * wgs, a path-1 launch wgs
 *     lds               dynamic LDS bytes per workgroup                                                                         */
typedef struct amdspeech_lstm_bidir_plan_info {
    int path, cus, fwd_kpw, fwd_waves, fwd_groups, fwd_wgs, fwd_lds, bwd_kpw, bwd_waves, bwd_groups, bwd_wgs, bwd_lds;
} amdspeech_lstm_bidir_plan_info;
int amdspeech_lstm_bidir_plan(const amdspeech_lstm_desc* d, amdspeech_lstm_bidir_plan_info* out);
int amdspeech_lstm_bidir_fwd(void* stream, const amdspeech_lstm_desc* d, void* ws, const float* const* kernels,
                             const float* const* biases, const int* lengths, const float* h0, const float* c0);
int amdspeech_lstm_bidir_bwd(void* stream, const amdspeech_lstm_desc* d, void* ws, const float* const* kernels,
                             float* const* dkernels, float* const* dbiases, const int* lengths);
int amdspeech_lstm_bidir_status(const amdspeech_lstm_desc* d, void* ws);
int amdspeech_lstm_bidir_dropout_multipliers(void* stream, const amdspeech_lstm_desc* d, int dir, int which, int layer, float* out);

/* ------------------------------------------------------------------- CTC ----
 * Replaces tf.nn.ctc_loss(sparse_labels, logits, seq_len,
 * ignore_longer_outputs_than_inputs=True) and its gradient,
 * models/AcousticModel.py:356-357, INCLUDING the label sparsification of
 * :155-159 / :174-178: `dense_labels` is the reference's labels_ph [B, U]
 * (0-padded); entries equal to 0 are dropped, an empty row becomes [C-1], the
 * target is every kept label before the first one >= C-1 (the blank / EOS),
 * required_time is the kept count; rows with lengths[b] == 0 or
 * required_time > lengths[b] get loss 0 and gradient 0.
 *   logits  [T,B,C]   loss [B]   dlogits [T,B,C] = d(sum_b loss_b)/dlogits   */
size_t amdspeech_ctc_workspace_bytes(int T, int B, int C, int U);
int amdspeech_ctc_loss_fwd_bwd(void* stream, const float* logits, const int* dense_labels,
                               const int* lengths, int T, int B, int C, int U,
                               float* loss, float* dlogits, void* ws);
/* The same in two calls, for a caller that wants to start other work on another stream in between: stage 1 = extended targets
 * + log-softmax into the workspace (short, fills the chip), stage 2 = the alpha / beta recursions and the gradient (long, 2 B
 * workgroups: most CUs are idle -- the product overlaps the next batch's front end here).  stage 0 = both (= the call above). */
int amdspeech_ctc_loss_fwd_bwd_staged(void* stream, const float* logits, const int* dense_labels,
                                      const int* lengths, int T, int B, int C, int U, float* loss,
                                      float* dlogits, void* ws, int stage);

/* The recursion kernel the call above takes for a shape, as plain numbers: a READ-ONLY view of the choice the launch itself reads
 * (one function decides for both).  Nothing is launched; the arguments are checked as the call checks them (C in 2 .. 4096,
 * U in 1 .. 2559: anything else is AMDSPEECH_EINVAL with a message, here and there).  Honours AMDSPEECH_CTC_SHIFT / AMDSPEECH_CTC_PAIR.
 *   kernel   AMDSPEECH_CTC_KERNEL_* below: WAVE one wavefront per (utterance, direction), up to 128 extended states; SHIFT the
 *            DPP-shift kernel with the float64 state (129 .. 384 states); PAIR two frames per LDS exchange (.. 512 states; the
 *            default from 385, and from 129 with AMDSPEECH_CTC_SHIFT=0); EDGE one LDS edge exchange per frame, `rmax` states per
 *            thread (2 only with AMDSPEECH_CTC_PAIR=0, 4 to 1024 states, 8 to 2048, 20 to 5119)
 *   threads  per (utterance, direction): 64 or 256;  rmax: states a thread can hold;  smax = 2 U + 1: pitch of the extended targets */
enum { AMDSPEECH_CTC_KERNEL_WAVE = 0, AMDSPEECH_CTC_KERNEL_SHIFT = 1, AMDSPEECH_CTC_KERNEL_PAIR = 2, AMDSPEECH_CTC_KERNEL_EDGE = 3 };
typedef struct amdspeech_ctc_plan_info {
    int kernel, threads, rmax, smax;
} amdspeech_ctc_plan_info;
int amdspeech_ctc_plan(int T, int B, int C, int U, amdspeech_ctc_plan_info* out);

/* Forced alignment: the best CTC alignment (Viterbi path) of a KNOWN transcript to the frames.  Same arguments, same label
 * sparsification, same limits and messages as amdspeech_ctc_loss_fwd_bwd; a workspace of its own (the loss's is untouched, so a
 * loss call and an alignment of the same logits may be queued back to back).
 *   v_t(s) = max(v_{t-1}(s), v_{t-1}(s-1), v_{t-1}(s-2) where the skip is legal) + log p_t(ext[s])   over the S = 2 n + 1
 * extended states, the state in float64 over the float32 log-softmax.  TIES go to the SMALLEST step (stay, then +1, then +2), and
 * at the last frame state S-1 wins over S-2: this rule is part of the contract.
 * Outputs, all DEVICE:
 *   frame_label [B][T]   the label emitted at each frame (C-1: blank), -1 for t >= lengths[b]
 *   frame_state [B][T]   the extended-state index at each frame, -1 for t >= lengths[b]
 *   spans       [B][U][2] first and last frame of every kept target label, in target order; -1 in unused slots
 *   score       [B]      natural-log probability of the best path; -inf where the target cannot be aligned (the loss is inf there);
 *                        0 for the rows the loss ignores (lengths[b] == 0 or required_time > lengths[b])
 *   confidence  [B][U]   exp(mean log p over the label's frames); 0 in unused slots
 * Rows with score 0 (ignored) or -inf have -1 in every frame and span.
 * Workspace (amdspeech_ctc_align_workspace_bytes; 256-byte aligned; each region rounded up to 256 bytes), in this order:
 *   log p  T*B*C*4 | extended targets  B*(2U+1)*4 | S  B*4 | valid  B*4 | final state  B*4 | best score  B*4 |
 *   back-pointers  B*T*pitch,  pitch = ceil((2U+1)/4) rounded up to 4: two bits per (frame, state)
 * amdspeech_ctc_align_plan: the recursion kernel a shape takes (one function decides for it and for the launch): WAVE, one
 * wavefront of two states per lane, up to 128 extended states; above that EDGE, 256 threads of `rmax` = 2 / 4 / 8 / 12 / 16 / 20 states
 * each (512 / 1024 / 2048 / 3072 / 4096 / 5119 states) with one LDS edge exchange per frame.  No run-time switch.                    */
size_t amdspeech_ctc_align_workspace_bytes(int T, int B, int C, int U);
int amdspeech_ctc_align_plan(int T, int B, int C, int U, amdspeech_ctc_plan_info* out);
int amdspeech_ctc_align(void* stream, const float* logits, const int* dense_labels, const int* lengths,
                        int T, int B, int C, int U, int* frame_label, int* frame_state, int* spans,
                        float* score, float* confidence, void* ws);

/* Greedy decode: per-frame argmax (first maximum), collapse repeats, drop the
 * blank C-1.  Stands where tf.nn.ctc_beam_search_decoder sits at
 * models/AcousticModel.py:312.  ids [B,T] is padded with C (the
 * reference pads its dense prediction with num_labels, :718); out_len [B].
 * ws: int32 scratch of T*B elements.                                          */
int amdspeech_ctc_greedy_decode(void* stream, const float* logits, const int* lengths,
                                int T, int B, int C, int* ids, int* out_len, int* ws);

/* In-place collapse of consecutive duplicate labels of each decoded row (ids [B,T], lens [B],
 * both DEVICE): TensorFlow's merge_repeated=True post-processing of the top path (:312).   */
int amdspeech_merge_repeated(void* stream, int* ids, int* lens, int T, int B, int pad);

/* Levenshtein distance of n_pairs sequence pairs on the device (replaces tf.edit_distance at
 * models/AcousticModel.py:370, un-normalised): a [n_pairs, lda], b [n_pairs, ldb], lengths per
 * pair, out int32 [n_pairs].                                                               */
int amdspeech_edit_distance(void* stream, const int* a, const int* a_len, int lda, const int* b,
                            const int* b_len, int ldb, int n_pairs, int* out);

/* HOST-side CTC prefix beam search (evaluation path): stands where
 * tf.nn.ctc_beam_search_decoder(logits, seq_len) (beam_width 100, top_paths 1,
 * merge_repeated True) sits at models/AcousticModel.py:312.  ALL pointers are HOST
 * memory: logits [T,B,C], lengths [B]; outputs ids [B,T] padded with C, out_len [B],
 * log_prob [B] (may be NULL).  merge_repeated != 0 collapses consecutive duplicate labels
 * of the returned path, as TensorFlow's default does.                                */
int amdspeech_ctc_beam_search_host(const float* logits, const int* lengths, int T, int B, int C,
                                   int beam_width, int merge_repeated, int* ids, int* out_len,
                                   float* log_prob);
/* The same with a cap on the decode threads of the call (max_threads <= 0: one per utterance, bounded by the core
 * count, as above): the asynchronous training-time decoder (rnn_speech_amd.acoustic_model._AsyncBeamDecoder) uses it to
 * keep a steady load on a few cores beside the training thread.                                                   */
int amdspeech_ctc_beam_search_host_mt(const float* logits, const int* lengths, int T, int B, int C,
                                      int beam_width, int merge_repeated, int* ids, int* out_len,
                                      float* log_prob, int max_threads);
/* The n-best list of the same search: the first n_best entries of the FINAL beam in the decoder's own total order (score
 * descending, then the prefixes in lexicographic order), so entry 0 is what the two calls above return, bit for bit.  ids
 * [B][n_best][T] padded with C, out_len [B][n_best], log_prob [B][n_best], n_found [B] (may be NULL) = min(n_best, beam entries);
 * unused slots get out_len 0 and log_prob -inf.  merge_repeated collapses each path on its own: two entries may then spell the
 * same ids (the caller that rescores them drops the duplicates).  All pointers HOST memory.                                  */
int amdspeech_ctc_beam_search_host_nbest(const float* logits, const int* lengths, int T, int B, int C,
                                         int beam_width, int merge_repeated, int n_best, int* ids, int* out_len,
                                         float* log_prob, int* n_found, int max_threads);

/* Levenshtein distance on the HOST (the same un-normalised tf.edit_distance as amdspeech_edit_distance, for predictions that
 * were decoded on the host: the asynchronous training-time beam decoder): all pointers HOST memory.                        */
int amdspeech_edit_distance_host(const int* a, const int* a_len, int lda, const int* b, const int* b_len, int ldb,
                                 int n_pairs, int* out);

/* CRC32C (Castagnoli) of a HOST buffer, continuing from `crc` (0 to start): the checksum
 * TensorFlow-bundle checkpoints carry per tensor and per table block (tf_bundle.py). */
uint32_t amdspeech_crc32c(const void* data, size_t n, uint32_t crc);

/* ------------------------------------------------------------- audio files ---
 * Host-side decode of RIFF/WAVE (PCM 8/16/24/32, IEEE float), FLAC (complete format, frame CRCs
 * always checked, STREAMINFO MD5 when verify != 0) and 16-bit PCM NIST SPHERE files to mono float32
 * in [-1, 1): the decode half of librosa.load(file) at util/audioprocessor.py:49 (channels averaged,
 * integer PCM scaled by 2^-(bits-1)).  `probe` reads the header only.  `decode` with out == NULL
 * reports frames / sample_rate; otherwise `capacity` must be >= frames.  HOST pointers.           */
int amdspeech_audio_probe(const char* path, int* sample_rate, int* channels, long* frames);
int amdspeech_audio_decode(const char* path, float* out, long capacity, long* frames, int* sample_rate,
                           int verify);

/* Resampler: the other half of librosa.load(file, sr=22050) at util/audioprocessor.py:49 -- band-limited
 * sinc interpolation with resampy's "kaiser_best" filter, on the GPU so that decoded PCM goes
 * H2D once and never comes back.  pcm [B, n_max] and out [B, out_max] are DEVICE buffers, n_samples a
 * HOST array; row b receives ceil(n_samples[b] * rate_out / rate_in) samples (amdspeech_resample_num_samples),
 * zero padded to out_max.
 * amdspeech_resample IS amdspeech_resample_rows (below: the definition of the arithmetic, the kernel and the workspace) with every
 * row at 1000 permille; amdspeech_resample_workspace_bytes(B) is amdspeech_resample_rows_workspace_bytes(B).  What follows from
 * that: a call with rate_in == rate_out COPIES its rows bit for bit and does not filter them; input at or past n_samples[b] is
 * not read and may hold anything; and the call refuses, with that call's messages, what that call refuses -- in particular a
 * ratio rate_out / rate_in outside 1/16 .. 16 (8 kHz .. 192 kHz audio into 16 or 22.05 kHz lies inside) and pcm / out ranges
 * that overlap.  Until the two calls shared a kernel this one had a kernel of its own that summed the same taps in another order: the
 * bits of resampled audio differ from that kernel's in the last places (either is within 2e-5 of the float64 oracle).            */
size_t amdspeech_resample_workspace_bytes(int B);
int amdspeech_resample_num_samples(int n_samples, int rate_in, int rate_out);
int amdspeech_resample(void* stream, const float* pcm, const int* n_samples, int B, int n_max, int rate_in,
                       int rate_out, float* out, int out_max, void* ws);

/* ------------------------------------------- per-row resampler / speed perturbation ---
 * The resampler: one kernel, a ratio of its own for every row, in ONE launch.  amdspeech_resample above is this call with every row
 * at 1000 permille; other speeds have no reference counterpart (an opt-in deviation, the three-way speed perturbation of Ko et al.
 * 2015 on the waveform, in front of the front end; off unless a caller asks for it).
 * A signal played f times faster is the signal resampled from rate * f to rate, so rate conversion and speed change are one pass.
 *   pcm            float [B][n_max] (DEVICE);  out  float [B][out_max] (DEVICE)
 *   n_samples      int32 [B] (HOST) valid samples per row, 0 .. n_max
 *   speed_permille int32 [B] (HOST) the row's speed in thousandths, 500 .. 2000 (0.5x .. 2.0x); 1000 = rate conversion only
 * Speed.  num = rate_out * 1000 and den = rate_in * speed_permille as 64-bit integers; ratio = (double)num / (double)den, ONE
 * double division of the two integers (at 1000 permille the same double as rate_out / rate_in).
 * Row lengths.  Row b receives n_total = ceil(n * num / den) samples, in exact integer arithmetic
 * (amdspeech_resample_rows_num_samples); a call with n_max * num >= 2^53 is refused.  Under that limit this equals
 * amdspeech_resample_num_samples' ceil((double)n * rate_out / rate_in) at 1000 permille.
 * Output arithmetic.  The first n_out = (int)((double)n * ratio) samples of a row are resampy's "kaiser_best" interpolation: the
 * table win[j] = kaiser(j) * rolloff * sinc(rolloff * j / 512), delta[j] = win[j + 1] - win[j] (stored WITHOUT the gain), scale = min(1, ratio),
 * step = (int)(scale * 512), and for output t:  tr = (double)t / ratio, k = (int)tr, frac = scale * (tr - k), off = (int)(frac * 512),
 * eta = frac * 512 - off; the left wing sums (win[off + i step] + eta delta[off + i step]) * x[k - i] over i < min(k + 1,
 * (32769 - off) / step), the right wing the same with frac' = scale - frac over x[k + 1 + i], i < min(n - k - 1, (32769 - off') / step)
 * -- the wing counts are clipped at both ends of the row; the two wing sums, each in tap order, are added and multiplied by the
 * row's gain (float)scale.  The remaining 0 or 1 samples up to n_total are +0.0f, and so are all samples from n_total to out_max.
 * Writes and reads.  The kernel writes EVERY word of out, so out may be uninitialised; it reads no input word at or past
 * n_samples[b], which may hold anything.
 * Copy rule.  A row with num == den (22,050 -> 22,050 at 1000, but also 44,100 -> 22,050 at 500) is COPIED bit for bit:
 * infinities, -0.0, denormals and NaN payloads arrive unchanged (the interpolation at ratio 1 is a low-pass, not the identity).
 * No atomics and no dependence on the launch order: two calls give the same bits.  Asynchronous on `stream`; lengths and speeds
 * travel as kernel arguments of one-block launches, 512 values each (2 B values: the lengths, then the speeds).
 *   ws   device, amdspeech_resample_rows_workspace_bytes(B) bytes, 256-byte aligned, caller-allocated: the table and the 2 B values
 * AMDSPEECH_EINVAL with a message: null pointers, non-positive B, n_max, out_max or rates, B > 65535, n_max * num >= 2^53, a
 * negative count or n > n_max, a permille outside 500 .. 2000, an out_max below a row's n_total, a ratio outside 1/16 .. 16, pcm and
 * out ranges that overlap.
 * amdspeech_resample_rows_plan: the launch geometry as plain numbers, a READ-ONLY view of the plan the call itself reads (one
 * function decides for both); no device is needed, the arguments are checked as the call checks them.
 *   tile           outputs per workgroup (1024: 256 threads of 4);  tiles_per_row = ceil(out_max / tile)
 *   workgroups     tiles_per_row * B: workgroup (x, b) owns outputs x * tile .. of row b.  A tile at or past n_total stores zeros,
 *                  a tile of a copy row copies (both branches are uniform over the workgroup), every other tile stages the input
 *                  span of its outputs in LDS once, then the table in chunks, and reads its taps and its table words from there
 *   span_max       the longest staged span in samples: over the rows with n > 0 and num != den the maximum of
 *                  min(n, (int)((tile - 1) / ratio) + 2 * (32769 / step) + 4);  0 when no row interpolates
 *   table_chunk    table entries (8 bytes each) a staged chunk holds: 4097, the taps i0 .. i0 + 4096 / step - 1 of every output;
 *                  0 when no row interpolates
 *   lds_bytes      dynamic LDS of the launch: 4 * span_max rounded up to 16, + 8 * table_chunk (37 KB at ratio 1, 51 KB at 1/4,
 *                  104 KB at the 1/16 bound)
 *   any_copy       1 when some row has num == den
 *   meta_launches  ceil(2 B / 512)
 * amdspeech_speed_perturb_draw: the speed of one utterance, host arithmetic with SpecAugment's integer hash (see there):
 *   idx = lo32(index) + hi32(index) * 0x9E3779B1 (32-bit wrap),  choice = (r(0x5B000000, idx) * count) >> 24,
 * returns factors_permille[choice] (count 1 .. 8, every factor 500 .. 2000; anything else is AMDSPEECH_EINVAL).             */
typedef struct amdspeech_resample_rows_plan_info {
    int tile, tiles_per_row, workgroups, span_max, table_chunk, lds_bytes, any_copy, meta_launches;
} amdspeech_resample_rows_plan_info;
int amdspeech_resample_rows_num_samples(int n_samples, int rate_in, int rate_out, int speed_permille);
size_t amdspeech_resample_rows_workspace_bytes(int B);
int amdspeech_resample_rows(void* stream, const float* pcm, const int* n_samples, const int* speed_permille, int B, int n_max,
                            int rate_in, int rate_out, float* out, int out_max, void* ws);
int amdspeech_resample_rows_plan(const int* n_samples, const int* speed_permille, int B, int n_max, int rate_in, int rate_out,
                                 int out_max, amdspeech_resample_rows_plan_info* out);
int amdspeech_speed_perturb_draw(unsigned long long seed, unsigned long long index, const int* factors_permille, int count);

/* ------------------------------------------------ noise and reverberation augmentation ---
 * Multi-condition training data (Ko et al. 2017) on the waveform, between the resampler and the front end, in the recipe's order:
 * speed perturbation -> reverberation by a room impulse response (RIR) -> additive noise at a drawn SNR -> features.  No reference
 * counterpart: an opt-in deviation, off unless a caller asks for it.  Three launches, all asynchronous on `stream`; the host-side
 * per-row values travel as kernel arguments of one-block launches, 512 values each (the resampler's hand-off), into `ws`.
 *
 * amdspeech_reverb_rows: a FIR with an impulse response of its own for every row, the whole batch in ONE launch.
 *   pcm        float [B][n_max] (DEVICE);  out  float [B][n_max] (DEVICE), a range that overlaps pcm (or rir_bank) is refused
 *   n_samples  int32 [B] (HOST)  valid samples per row, 0 .. n_max
 *   rir_bank   float [R][taps_max] (DEVICE)  row r holds h_r[0 .. rir_taps[r]); words past that are not read
 *   rir_taps   int32 [R] (HOST)  L, 1 .. taps_max;  taps_max <= 8192
 *   rir_delay  int32 [R] (HOST)  d, 0 .. L - 1: the position of the direct path, so that speech stays aligned with its labels
 *   rir_index  int32 [B] (HOST)  -1 .. R - 1: the row's impulse response, -1 = none
 * For a row with r = rir_index[b] >= 0 and 0 <= t < n:   out[b][t] = sum_{k = 0 .. L - 1} h_r[k] * x_b[t + d - k]   over the terms
 * with 0 <= t + d - k < n only.  The output is as long as the input (the reverberant tail past n is dropped), out[b][n .. n_max) is
 * +0.0f, input words at or past n_samples[b] are not read and may hold anything, every word of out is written.  A row with
 * rir_index -1 is COPIED bit for bit (NaN payloads, -0.0).
 * Arithmetic.  The sum is a matrix product on the f32 matrix cores (v_mfma_f32_32x32x2_f32, exact f32: an fmaf chain).  For a tile
 * of 1024 outputs t = t0 + 32 i + j:  Y[i][j] = sum_q X[i][q] G[q][j] with X[i][q] = x[t0 + d - (L - 1) + 32 i + q] and
 * G[q][j] = h[j + L - 1 - q] (0 outside 0 .. L - 1), q = 0 .. 32 * k_chunks - 1.  q runs in chunks of 32; the four waves of the
 * workgroup take the chunks round-robin (wave w: chunks w, w + 4, ..), each summing its terms in q order from +0.0f, and the four
 * partial sums are added ((w0 + w1) + w2) + w3.  So the order is fixed -- no atomics, no dependence on the launch order, two calls
 * give the same bits -- and every output is within (L + 2) * 2^-24 * sum_k |h[k] x[t + d - k]| of the exact sum.  The zero frame of
 * G multiplies staged samples up to 31 positions beyond an output's own reach: the samples of a filtered row must be FINITE (an
 * infinity inside a row turns outputs within L + 31 of it into NaN, 31 more than the sum itself would).
 *   ws   device, amdspeech_reverb_rows_workspace_bytes(B) bytes, 256-byte aligned, caller-allocated: 4 B values
 * AMDSPEECH_EINVAL with a message: null pointers, non-positive B, n_max, R or taps_max, B > 65535, n_max > 2^30, taps_max > 8192, taps
 * outside 1 .. taps_max, a delay outside 0 .. taps - 1, a negative count or n > n_max, an index outside -1 .. R - 1, overlapping ranges.
 * amdspeech_reverb_rows_plan: the launch geometry as plain numbers, a READ-ONLY view of the plan the call itself reads (one function
 * decides for both); no device is needed, the arguments are checked as the call checks them.
 *   tile           outputs per workgroup (1024: 32 x 32, one MFMA tile);  tiles_per_row = ceil(n_max / tile)
 *   workgroups     tiles_per_row * B: workgroup (x, b) owns outputs x * tile .. of row b.  A tile at or past n stores zeros, a tile
 *                  of a copy row copies (both branches are uniform over the workgroup)
 *   taps           the longest impulse response among the rows with an index >= 0 and n > 0;  0: every row copies
 *   k_chunk        32: values of q per step of a wave;  k_chunks = ceil((taps + 31) / 32)
 *   span_max       staged input samples of a tile: tile - 32 + 32 * k_chunks (0 when taps is 0)
 *   lds_bytes      dynamic LDS of the launch: the span with one pad word per 32, rounded up to 16 bytes and at least 16 KB (the four
 *                  partial tiles reuse it), then 32 * k_chunks + 32 reversed, zero-framed taps (69 KB at 8192 taps: two
 *                  workgroups a CU; 37 KB at 4096)
 *   copy_rows      rows with rir_index -1
 *   meta_launches  ceil(4 B / 512)
 *
 * amdspeech_row_sumsq: sumsq[b] = sum_{t < n} x[b][t]^2 as float64 (DEVICE, [B]); pcm, n_samples as above, words at or past n are
 * not read.  Fixed tiles, fixed order, no atomics: the row is cut into tiles of 4096 samples, workgroup s of the row's 64 takes tiles
 * s, s + 64, .. in order, thread i of 256 adding x^2 (fma in double) of words i, i + 256, .. of each tile to its own sum; the 256 sums
 * are added pairwise (i with i + 128, then + 64, ..), and so are the 64 partial sums.  The bits depend on the row and n alone, not on
 * B, n_max or the call.  n = 0 gives 0.0.  ws: amdspeech_row_sumsq_workspace_bytes(B) bytes (64 B doubles, B values), 256-byte aligned.
 * EINVAL: null pointers, non-positive B or n_max, B > 65535, n_max > 2^30, a negative count or n > n_max.
 *
 * amdspeech_noise_mix_rows: one launch; out == pcm (in place) is allowed, a partial overlap is refused.
 *   noise_bank   float [M][m_max] (DEVICE);  noise_len  int32 [M] (HOST) 1 .. m_max;  noise_sumsq  double [M] (DEVICE), the
 *                amdspeech_row_sumsq of the clips
 *   row_sumsq    double [B] (DEVICE), the amdspeech_row_sumsq of pcm
 *   noise_index  int32 [B] (HOST) -1 .. M - 1, -1 = none;  noise_offset  int32 [B] (HOST) 0 .. len - 1;
 *   snr_decidb   int32 [B] (HOST) -200 .. 600: the signal-to-noise ratio in tenths of a dB (offset and SNR of a -1 row are not read)
 * For a row with m >= 0, n > 0, row_sumsq[b] > 0 and noise_sumsq[m] > 0 the gain is computed in double and rounded once,
 *   g = (float) sqrt((row_sumsq[b] / n) / (noise_sumsq[m] / len_m) * p),   p = pow(10.0, -snr_decidb / 100.0) on the HOST,
 * and  out[b][t] = fmaf(g, noise_m[(offset + t) mod len_m], x[b][t])  for t < n: a short clip wraps around.  Every other row is
 * copied bit for bit (left alone when in place).  Words at or past n are not read; out of place they are written +0.0f, in place
 * they are left alone (the zeros the resampler or the reverberation left stay).
 *   ws   amdspeech_noise_mix_rows_workspace_bytes(B) bytes, 256-byte aligned: 6 B values
 * EINVAL: null pointers, non-positive B, n_max, M or m_max, B > 65535, n_max or m_max > 2^30, a length outside 1 .. m_max, a negative
 * count or n > n_max, an index outside -1 .. M - 1, an offset outside 0 .. len - 1, an SNR outside -200 .. 600, overlapping ranges.
 * amdspeech_noise_mix_rows_plan: as above;  tile 1024 (256 threads of 4), tiles_per_row, workgroups = tiles_per_row * B, lds_bytes 0,
 * copy_rows the rows with noise_index -1, meta_launches ceil(6 B / 512).
 *
 * amdspeech_augment_draw: what happens to one utterance, host arithmetic with SpecAugment's integer hash r (see there):
 *   idx = lo32(index) + hi32(index) * 0x9E3779B1 (32-bit wrap),   u(s, count) = (r(0x5C000000 + s, idx) * count) >> 24  (64-bit product)
 *   out[0] rir_index     R > 0 and u(0, 1000) < reverb_permille ?  u(1, R)  : -1
 *   out[1] noise_index   M > 0 and u(2, 1000) < noise_permille  ?  u(3, M)  : -1
 *   out[2] noise_offset  u(4, noise_len[noise_index]);   out[3] snr_decidb  snr_lo + u(5, snr_hi - snr_lo + 1)   (both 0 without noise)
 * EINVAL: a null out (or noise_len with M > 0), a probability outside 0 .. 1000 permille, a negative R or M, a length below 1, an SNR
 * range that is empty or outside -200 .. 600.                                                                                  */
typedef struct amdspeech_reverb_rows_plan_info {
    int tile, tiles_per_row, workgroups, taps, span_max, k_chunk, k_chunks, lds_bytes, copy_rows, meta_launches;
} amdspeech_reverb_rows_plan_info;
typedef struct amdspeech_noise_mix_rows_plan_info {
    int tile, tiles_per_row, workgroups, lds_bytes, copy_rows, meta_launches;
} amdspeech_noise_mix_rows_plan_info;
size_t amdspeech_reverb_rows_workspace_bytes(int B);
int amdspeech_reverb_rows(void* stream, const float* pcm, const int* n_samples, int B, int n_max, const float* rir_bank,
                          const int* rir_taps, const int* rir_delay, int R, int taps_max, const int* rir_index, float* out, void* ws);
int amdspeech_reverb_rows_plan(const int* n_samples, int B, int n_max, const int* rir_taps, const int* rir_delay, int R, int taps_max,
                               const int* rir_index, amdspeech_reverb_rows_plan_info* out);
size_t amdspeech_row_sumsq_workspace_bytes(int B);
int amdspeech_row_sumsq(void* stream, const float* pcm, const int* n_samples, int B, int n_max, double* sumsq, void* ws);
size_t amdspeech_noise_mix_rows_workspace_bytes(int B);
int amdspeech_noise_mix_rows(void* stream, const float* pcm, const int* n_samples, int B, int n_max, const float* noise_bank,
                             const int* noise_len, const double* noise_sumsq, int M, int m_max, const double* row_sumsq,
                             const int* noise_index, const int* noise_offset, const int* snr_decidb, float* out, void* ws);
int amdspeech_noise_mix_rows_plan(const int* n_samples, int B, int n_max, const int* noise_len, int M, int m_max,
                                  const int* noise_index, const int* noise_offset, const int* snr_decidb,
                                  amdspeech_noise_mix_rows_plan_info* out);
int amdspeech_augment_draw(unsigned long long seed, unsigned long long index, int reverb_permille, int R, int noise_permille, int M,
                           const int* noise_len, int snr_lo_decidb, int snr_hi_decidb, int* out);

/* ------------------------------------------------------------- optimiser ----
 * Replaces tf.clip_by_global_norm + tf.train.AdamOptimizer.apply_gradients over
 * the flat parameter vector, models/AcousticModel.py:388 and :404-406.
 *   g' = g * clip / max(||g||_2, clip)
 *   m = b1 m + (1-b1) g' ; v = b2 v + (1-b2) g'^2 ; p -= lr_t m / (sqrt(v) + eps)
 * lr_t = lr*sqrt(1-b2^t)/(1-b1^t) is formed by the caller.  norm_out (device,
 * 1 float) receives ||g||_2.  ws: float scratch of
 * amdspeech_optim_workspace_bytes(n) bytes.                                   */
size_t amdspeech_optim_workspace_bytes(long n);
int amdspeech_clip_adam(void* stream, float* params, const float* grads, float* m, float* v,
                        long n, float clip, float lr_t, float beta1, float beta2, float eps,
                        float* norm_out, void* ws);

/* -------------------------------------------------------------- front end ---
 * Replaces AudioProcessor._extract_mfcc (librosa.feature.mfcc,
 * util/audioprocessor.py:63-75) and AudioProcessor._extract_fbank
 * (util/audioprocessor.py:77-161) for a batch of utterances.
 *   pcm        float [B][n_max]  mono samples, rows zero-padded
 *   n_samples  int32 [B] (HOST) valid samples per row
 *   feat       float [t_max][B][D] time-major, zero past each utterance's frames
 *   n_frames   int32 [B] (HOST, out) UNtruncated frame counts (reference quirk:
 *              the returned length is not clipped to max_input_seq_length)
 * mfcc: D = n_mfcc (reference default 20).  fbank: D = 120.                   */
size_t amdspeech_frontend_workspace_bytes(int mode, int B, int n_max, int sample_rate);
int amdspeech_frontend_num_frames(int mode, int n_samples, int sample_rate);
int amdspeech_frontend_mfcc(void* stream, const float* pcm, const int* n_samples, int B,
                            int n_max, int sample_rate, int n_mfcc, int t_max,
                            float* feat, int* n_frames, void* ws);
int amdspeech_frontend_fbank(void* stream, const float* pcm, const int* n_samples, int B,
                             int n_max, int sample_rate, int t_max,
                             float* feat, int* n_frames, void* ws);

/* The kernels the two calls above take for a shape, as plain numbers: a READ-ONLY view of the plan the launch itself reads (one
 * function decides for both).  Nothing is launched and no device is needed; the arguments are checked as the calls check them
 * (mode 0 mfcc / 1 fbank, B, n_max, t_max > 0, sample_rate >= 1000 and a DFT of at most 2048 points, n_mfcc in 1 .. 128 for mfcc:
 * anything else is AMDSPEECH_EINVAL with a message, here and there).  Honours AMDSPEECH_FRONTEND_MFMA (read once per process).
 *   frames_kernel  0 the vector-ALU frame kernel (8 frames per workgroup), 1 the matrix-core one (a queue of 32-frame tiles).  The
 *                  choice is by LDS bytes: the matrix-core kernel needs (64 (kp + 4) + 31 hop + frame_len) * 4 <= 163,584, which
 *                  holds for mfcc below 35.75 kHz and for fbank below 69.95 kHz; AMDSPEECH_FRONTEND_MFMA=0 takes kernel 0 everywhere
 *   maxq           bin tiles a wave of the matrix-core kernel can own: 4 (up to 16 tiles), 5 (up to 20), 9 (above); 0 for kernel 0
 *   n_dft, frame_len, hop, n_bins   DFT points (mfcc: round(0.025 rate); fbank: 512), window samples kept, samples between frames
 *   bin_tiles, kp  16-bin tiles of the spectrum, padded length of the folded frame (multiples of 16 / 32)
 *   lds_bytes      dynamic LDS of the frame kernel that is launched
 *   t_full         frames of an n_max-sample row (the pitch of the workspace)
 *   tiles_per_utt, n_items, workgroups   kernel 1: 32-frame tiles per row, queue items (tiles_per_utt * B), workgroups that drain
 *                  the queue (at most 512);  kernel 0: grid x (8-frame tiles per row), grid x * grid y (y = B), and the same again
 *   dct_kernel     -1 fbank (no DCT), 0 the vector-ALU DCT, 1 the matrix-core DCT;  dct_col_tiles: its 16-coefficient column tiles
 *   meta_by_copy   1 when B > 256: the lengths reach the device by a copy and a stream synchronisation, not as kernel arguments */
typedef struct amdspeech_frontend_plan_info {
    int frames_kernel, maxq, n_dft, frame_len, hop, n_bins, bin_tiles, kp, lds_bytes, t_full, tiles_per_utt, n_items, workgroups, dct_kernel, dct_col_tiles, meta_by_copy;
} amdspeech_frontend_plan_info;
int amdspeech_frontend_plan(int mode, int sample_rate, int n_mfcc, int B, int n_max, int t_max,
                            amdspeech_frontend_plan_info* out);

/* ---------------------------------------------------- low frame rate input ---
 * Frame stacking and subsampling between the front end and the input Linear (no reference counterpart: an opt-in deviation,
 * off when stack = skip = 1, where no caller makes this call): `stack` consecutive front-end frames are concatenated into one
 * model frame and every `skip`-th such frame is kept.  With the input Linear behind it this is a strided 1-D convolution over
 * time; everything past it runs ceil(T / skip) frames.
 *   x         float [t_in][B][D]   the front end's `feat`, time-major
 *   n_frames  int32 [B] (HOST)     the front end's UNtruncated frame counts: n_frames[b] may exceed t_in
 *   out       float [t_out][B][stack * D],  t_out = ceil(t_in / skip)
 *   n_out     int32 [B] (HOST, out) ceil(n_frames[b] / skip), untruncated in the same way
 *   out[j][b][i * D + d] = x[j * skip + i][b][d]   if j * skip + i < min(n_frames[b], t_in),   0 otherwise
 * The kernel writes EVERY element of out (a row past its utterance is all zeros), masks by n_frames[b] itself -- frames of x at or
 * past it are never read and may hold anything -- and copies bit patterns: -0.0, denormals, infinities and NaN payloads of the
 * valid region arrive unchanged.  Asynchronous on `stream`; the lengths travel as kernel arguments up to 256 rows, above that
 * through a device buffer of the call's own (the call then waits for the stream before it returns).
 * AMDSPEECH_EINVAL with a message: null pointers, non-positive sizes, a negative count, stack or skip outside 1 .. 16,
 * stack * D > 4096, x and out ranges that overlap, and -- when D is a multiple of 4 (16-byte loads and stores) -- a base pointer
 * that is not 16-byte aligned.
 * amdspeech_frame_stack_num_frames: ceil(n_frames / skip), host arithmetic (AMDSPEECH_EINVAL for n_frames < 0 or a bad skip).
 * amdspeech_frame_stack_plan: the launch geometry as plain numbers, a READ-ONLY view of the plan the launch itself reads (one
 * function decides for both); no device is needed, the shape is checked as the call checks it.
 *   t_out, d_out   ceil(t_in / skip), stack * D
 *   vec            words per lane and access: 4 when D % 4 == 0, else 1
 *   workgroups     of 256 threads; the smallest power of two of lanes that covers d_out / vec (at most 256) shares one
 *                  (model frame, row) item, the grid strides over the items and is capped at 2048
 *   meta_by_copy   1 when B > 256                                                                                              */
typedef struct amdspeech_frame_stack_plan_info {
    int t_out, d_out, vec, workgroups, meta_by_copy;
} amdspeech_frame_stack_plan_info;
int amdspeech_frame_stack_num_frames(int n_frames, int skip);
int amdspeech_frame_stack(void* stream, const float* x, const int* n_frames, int B, int D, int t_in, int stack, int skip,
                          float* out, int* n_out);
int amdspeech_frame_stack_plan(int B, int D, int t_in, int stack, int skip, amdspeech_frame_stack_plan_info* out);

/* ------------------------------------------------------------ SpecAugment ----
 * Frequency and time masks on a training mini-batch's features, IN PLACE, between the front end (or the frame stacking) and the
 * model (no reference counterpart: an opt-in deviation; time warping is not part of it, speed perturbation is amdspeech_resample_rows).  The input
 * needs no gradient, so there is no backward call: the input Linear's weight gradient simply reads the masked tensor.
 *   x        float [T][B][W]      time-major, contiguous; masked words become +0.0f, every other word keeps its bit pattern
 *   lengths  int32 [B] (DEVICE)   frames of each row; n_b = min(lengths[b], T); a row with n_b <= 0 is not touched, and no
 *                                 frame at or past n_b is written
 * The policy:
 *   period         P: channels of one source frame's frequency axis; W % P == 0 and channel c belongs to bin c % P
 *                  (fbank: 40, so a mel bin is masked in the static, delta and delta-delta groups together; under frame
 *                  stacking the source frame's bin count, so a bin is masked in every stacked sub-frame; mfcc: n_mfcc).
 *                  1 <= P <= W <= 4096
 *   freq_masks     F frequency masks per row, 0 .. 8;   freq_width  Fw: their largest width in bins, 0 .. P
 *   time_masks     M time masks per row, 0 .. 16;       time_width  Tw: their largest width in frames, >= 0
 *   time_permille  0 .. 1000: no time mask is wider than n_b * time_permille / 1000 frames (integer division)
 *   seed           64 bits
 * The draws, in integer arithmetic only (the host, the device and a restatement in another language agree exactly):
 *   r(stream, idx) = mix32(mix32(idx ^ lo32(seed)) + stream * 0x9e3779b9 + hi32(seed)) >> 8          (24 bits),
 *   mix32(v): v ^= v >> 16; v *= 0x7feb352d; v ^= v >> 15; v *= 0x846ca68b; v ^= v >> 16    (32-bit wrap-around)
 *   mask m of row b: idx = b * 64 + m, stream = 0x5A000000 + 2 * kind + which (kind 0 frequency, 1 time; which 0 width, 1 start)
 *   wmax   = kind == 0 ? min(Fw, P) : min(Tw, n_b * time_permille / 1000)        extent = kind == 0 ? P : n_b
 *   width  = (r(width stream, idx) * (wmax + 1)) >> 24                 0 .. wmax             (64-bit products)
 *   start  = (r(start stream, idx) * (extent - width + 1)) >> 24       0 .. extent - width
 * Element (t, b, c) with t < n_b becomes +0.0f when c % P lies in a frequency span of row b or t lies in a time span of row b.
 * The kernel is write-only: it reads the lengths and its arguments and stores zeros to the masked words; it loads nothing from x.
 * Asynchronous on `stream`, no host copy, no synchronisation.  When neither kind can mask anything (F or Fw is 0, and M, Tw or
 * time_permille is 0) nothing is launched.
 * AMDSPEECH_EINVAL with a message: null pointers, non-positive T or B (or T * B >= 2^31), W outside 1 .. 4096, a period outside 1 .. W or one that
 * does not divide W, F outside 0 .. 8, M outside 0 .. 16, Fw outside 0 .. P, a negative Tw, time_permille outside 0 .. 1000.
 * amdspeech_spec_augment_spans: the spans of one row as the kernel draws them (host arithmetic, the same function the kernel
 * calls): 2 * (F + M) ints, (start, width) pairs, the F frequency masks first; `n` is the row's n_b (>= 0; period, not W,
 * bounds the frequency spans, so no W is passed and the period is only checked against 1 .. 4096).
 * amdspeech_spec_augment_plan: the launch geometry as plain numbers, a READ-ONLY view of the plan the launch itself reads (one
 * function decides for both); no device is needed, the shape and the policy are checked as the call checks them.
 *   vec                 words per store of a time-masked frame: 4 when W % 4 == 0 (the query assumes a 16-byte aligned x; the
 *                       call plans with 1 when x is not), else 1.  Frequency spans start at any word: single-word stores
 *   lanes               threads that share one (frame, row) item: the smallest power of two that covers the W / vec stores of a
 *                       whole frame at 4 stores per lane, at most 256
 *   items_per_workgroup 256 / lanes
 *   workgroups          of 256 threads, at most 2048 (the grid strides over the T * B items); 0 = nothing is launched
 *   reps                W / period                                                                                         */
typedef struct amdspeech_spec_augment_desc {
    int period, freq_masks, freq_width, time_masks, time_width, time_permille;
    unsigned long long seed;
} amdspeech_spec_augment_desc;
typedef struct amdspeech_spec_augment_plan_info {
    int vec, lanes, items_per_workgroup, workgroups, reps;
} amdspeech_spec_augment_plan_info;
int amdspeech_spec_augment(void* stream, float* x, const int* lengths, int T, int B, int W,
                           const amdspeech_spec_augment_desc* desc);
int amdspeech_spec_augment_spans(const amdspeech_spec_augment_desc* desc, int row, int n, int* spans);
int amdspeech_spec_augment_plan(int T, int B, int W, const amdspeech_spec_augment_desc* desc,
                                amdspeech_spec_augment_plan_info* out);

/* ---------------------------------------------------- feature normalisation ---
 * Cepstral mean and variance normalisation of the front end's features, IN PLACE, between the front end and the frame stacking
 * (no reference counterpart: an opt-in deviation, off in mode 0, where no caller makes this call).  The input needs no gradient,
 * so there is no backward call.
 *   x         float [t_in][B][D]   the front end's `feat`, time-major, contiguous; D <= 4096
 *   n_frames  int32 [B] (HOST)     the front end's UNtruncated frame counts; n = min(n_frames[b], t_in)
 * For row b and dim d, over the frames t < n only:
 *   mean = (1/n) sum x[t][b][d]        var = (1/n) sum (x[t][b][d] - mean)^2        (the POPULATION variance)
 *   x[t][b][d] = float((double(x[t][b][d]) - mean) * scale),    scale = norm_vars ? 1 / sqrt(max(var, var_floor)) : 1
 * Frames at or past n are neither read nor written; a row with n = 0 is not touched; a row with n = 1 becomes zeros.  A constant
 * dim has var = 0 and x - mean = 0 exactly: it comes out as exact zeros.
 * Modes (amdspeech_feature_norm_desc.mode):
 *   AMDSPEECH_FEATURE_NORM_NONE       nothing is launched
 *   AMDSPEECH_FEATURE_NORM_UTTERANCE  mean and var of the row itself
 *   AMDSPEECH_FEATURE_NORM_GLOBAL     one (mean[d], scale[d]) for all rows from `table`, double [2][D] on the DEVICE (mean first);
 *                                     norm_vars and var_floor are then already folded into the table and are not read
 * The arithmetic (utterance mode): accumulation is in float64, shifted by the row's own first frame K[d] = x[0][b][d]:
 *   S' = sum (x - K),  Q' = sum (x - K)^2,  mean = K + S'/n,  var = max(Q'/n - (S'/n)^2, 0)
 * The shift is the same for every time slice of a row, so the partial sums of the `split` workgroups of a row add directly; it
 * makes a constant dim exactly zero-variance and keeps the single pass accurate when |mean| >> std.  scale is formed in float64;
 * the result is rounded to float ONCE.  No atomics: partial sums are combined in a fixed order, two calls give the same bits.
 * Global mode performs the same two float64 operations and the one rounding on the table's values: bit for bit
 * float32((float64(x) - mean) * scale).
 * Asynchronous on `stream`; the lengths travel as kernel arguments up to 256 rows, above that through a device buffer of the
 * call's own (the call then waits for the stream before it returns).
 *   workspace  device, amdspeech_feature_norm_plan_info.workspace_bytes of the UTTERANCE plan (8-byte aligned), caller-allocated;
 *              may be NULL in global mode.  Per row: `split` partials double [2][D] (S', Q') and the row's K double [D]
 * amdspeech_feature_moments: the same sums, finished per row instead of applied -- moments is a device double [B][2][D] holding
 * mean and M2 = sum (x - mean)^2 (zeros for n = 0); x is not written.  The building block of corpus statistics: rows merge on the
 * host with the pairwise update.  Takes the workspace of the utterance plan.
 * AMDSPEECH_EINVAL with a message: null pointers, non-positive sizes (or t_in * B >= 2^31), D > 4096, a mode outside 0 .. 2,
 * var_floor <= 0, NaN or infinite, a negative count, float64 buffers that are not 8-byte aligned, and -- when D is a multiple
 * of 4 (16-byte loads and stores) -- an x that is not 16-byte aligned: such a base is REFUSED, not run with single-word accesses.
 * amdspeech_feature_norm_plan: the launch geometry as plain numbers, a READ-ONLY view of the plan the launches themselves read (one
 * function decides for both); no device is needed, the shape is checked as the calls check it.
 *   vec              words per lane and access: 4 when D % 4 == 0, else 1
 *   split            time slices per row = workgroups per row.  Chosen from t_in, B and D alone: ceil(512 / min(B, 2048)) so that a
 *                    small batch still covers the chip, but no more than floor(t_in / (4 * slots)) -- a slice is no shorter
 *                    than 4 passes of the 256 / lanes frame slots, lanes = the smallest power of two that covers D / vec (at
 *                    most 256) -- and at least 1; then re-derived as ceil(t_in / ceil(t_in / split)) so that no slice is empty
 *   workgroups       split * min(B, 2048), of 256 threads (rows beyond 2048 are strided); 0 in mode 0
 *   lds_bytes        static LDS of either kernel: 256 * 2 * vec doubles
 *   meta_by_copy     1 when B > 256
 *   workspace_bytes  B * (2 * split + 1) * D * 8 in utterance mode, 0 otherwise                                              */
#define AMDSPEECH_FEATURE_NORM_NONE 0
#define AMDSPEECH_FEATURE_NORM_UTTERANCE 1
#define AMDSPEECH_FEATURE_NORM_GLOBAL 2
typedef struct amdspeech_feature_norm_desc {
    int mode, norm_vars;
    double var_floor;
} amdspeech_feature_norm_desc;
typedef struct amdspeech_feature_norm_plan_info {
    int vec, split, workgroups, lds_bytes, meta_by_copy, workspace_bytes;
} amdspeech_feature_norm_plan_info;
int amdspeech_feature_norm_plan(int B, int D, int t_in, int mode, amdspeech_feature_norm_plan_info* out);
int amdspeech_feature_moments(void* stream, const float* x, const int* n_frames, int B, int D, int t_in, void* workspace,
                              double* moments);
int amdspeech_feature_norm(void* stream, float* x, const int* n_frames, int B, int D, int t_in,
                           const amdspeech_feature_norm_desc* desc, const double* table, void* workspace);

/* ------------------------------------------------------ lookahead convolution ---
 * A row convolution above the top layer of a UNIDIRECTIONAL LSTM stack (Deep Speech 2's "lookahead convolution"; no reference
 * counterpart: an opt-in deviation, off at context 0, where no caller makes these calls and no parameter exists): a depth-wise
 * filter over the next `context` frames, one weight per future frame and hidden unit.  (context + 1) * H parameters, no bias, no
 * activation.
 *   x, y, dy, dx  float [T][B][H]        time-major, contiguous
 *   w, dw         float [context + 1][H]
 *   lengths       int32 [B] (DEVICE)     frames of each row;  Lb = min(lengths[b], T), a negative length counts as 0
 *   context       1 .. 32
 *   fwd:  y[t][b][h]  = sum_{j = 0 .. context, t + j < Lb} w[j][h] * x[t + j][b][h]      for t < Lb,   0 for t >= Lb
 *   bwd:  dx[t][b][h] = sum_{j = 0 .. context, t - j >= 0} w[j][h] * dy[t - j][b][h]     for t < Lb,   0 for t >= Lb
 *         dw[j][h]   += sum_b sum_{t, t + j < Lb} dy[t][b][h] * x[t + j][b][h]            (ACCUMULATES, as amdspeech_linear_bwd does)
 * The arithmetic: every element of y and dx is ONE chain of fmaf in ascending j that starts from the rounded product of the j = 0
 * tap; taps outside the row are not added at all (they are not zeros that take part).  With w[0] = 1 and w[j > 0] = 0, y therefore
 * equals x as numbers wherever t < Lb.  dw is summed in three fixed stages: per (time chunk, row b) one fmaf chain in ascending t
 * over the at most `dw_terms` frames of the chunk (a partial [context + 1][H] tile in the workspace); per element `reduce_slices`
 * plain float sums, each over a contiguous run of at most `reduce_terms` partials in index order (index = chunk * B + b); the slices
 * added in slice order, and one add into dw.  No floating-point atomics anywhere: y, dx and dw are bit-identical from run to run
 * and do not depend on what else the chip is doing.
 * y and dx are written in EVERY element; frames of x and dy at or past Lb are never read and may hold anything (NaN included).
 * The workspace is written in every word the second stage reads: it needs no fill.  Asynchronous on `stream`; nothing is copied to
 * the host.  Three launches backward (dx, the dw partials, their sum), one forward.
 * Each kernel walks time with a sliding window of context + 1 frames in LDS: a frame is loaded from memory once per time chunk, and
 * a chunk re-reads only its halo of `context` frames (at most a quarter of `t_chunk`).
 * AMDSPEECH_EINVAL with a message and no launch: null pointers (the workspace included), non-positive sizes, B * H or T * B >= 2^31,
 * a context outside 1 .. 32, x / y ranges that overlap (fwd), dy / dx or x / dx ranges that overlap (bwd).
 * amdspeech_lookahead_bwd_workspace_bytes: bytes of `ws` (device, caller-allocated, 16-byte aligned for the 16-byte path); 0 for a
 * shape the calls refuse.  The figure covers the shape and every SHORTER T at the same B, H and context (a caller sizes it once
 * for its padded length): min(ceil(1024 / col_blocks), ceil(T / the chunk floor)) * B tiles of (context + 1) * H floats, which is
 * at least dw_partials tiles.
 * amdspeech_lookahead_plan: the launch geometry as plain numbers, a READ-ONLY view of the plan the launches themselves read (one
 * function decides for all of them); no device is needed, the shape is checked as the calls check it.
 *   vec                words per lane and access: 4 when H % 4 == 0, else 1.  The query assumes 16-byte aligned bases; a call whose
 *                      x, w, y (bwd: x, w, dy, dx, ws) are not all 16-byte aligned plans with 1 instead -- its chunks are then no
 *                      more than the query's, so the queried workspace still covers it
 *   unroll             frames per block of the walk = independent loads in flight per lane (8)
 *   col_blocks         workgroups along a [B][H] frame: ceil(B * H / vec / 64), 64 threads each, lanes along the frame
 *   t_chunk, chunks    frames per time chunk, the same for all three walks: ceil(T / ceil(1024 / col_blocks)) so that the grid covers
 *                      the chip, but at least 4 * context, rounded up to whole blocks;  chunks = ceil(T / t_chunk)
 *   workgroups         col_blocks * chunks: of the forward launch, of the dx launch and of the dw-partials launch
 *   lds_bytes          dynamic LDS of each of those: (2 * context + unroll + 1) * 64 * vec * 4 -- the window ring and, beside it,
 *                      the lane's weights (fwd, dx) or its running dw sums
 *   dw_partials        partial dw tiles in the workspace = chunks * B;   dw_terms: frames summed into one = t_chunk
 *   reduce_slices      threads per dw element in the second stage (8);   reduce_terms: partials per slice = ceil(dw_partials / 8)
 *   reduce_workgroups  of 256 threads: ceil((context + 1) * H / 32)                                                              */
typedef struct amdspeech_lookahead_plan_info {
    int vec, unroll, col_blocks, t_chunk, chunks, workgroups, lds_bytes, dw_partials, dw_terms, reduce_slices, reduce_terms, reduce_workgroups;
} amdspeech_lookahead_plan_info;
int amdspeech_lookahead_fwd(void* stream, const float* x, const float* w, const int* lengths, int T, int B, int H, int context,
                            float* y);
size_t amdspeech_lookahead_bwd_workspace_bytes(int T, int B, int H, int context);
int amdspeech_lookahead_bwd(void* stream, const float* x, const float* w, const float* dy, const int* lengths, int T, int B, int H,
                            int context, float* dx, float* dw, void* ws);
int amdspeech_lookahead_plan(int T, int B, int H, int context, amdspeech_lookahead_plan_info* out);

/* ------------------------------------------- time-frequency convolution (front) ---
 * A strided 2-D convolution between the features and the input Linear (Deep Speech 2's convolutional front; no reference
 * counterpart: an opt-in deviation, off at 0 channels, where no caller makes these calls and no parameter exists).  "Same" padding,
 * pt = (kt - 1) / 2, pf = (kf - 1) / 2; the clipped ReLU min(max(., 0), 20).  First layer of the model: there is no dx.
 *   x             float [T][B][G][F]     the front end's frame seen as G groups of F bins (fbank: 3 x 40, mfcc: 1 x n_mfcc)
 *   w, dw         float [K][C]           K = G * kt * kf, row k = (g * kt + i) * kf + j
 *   bias, db      float [C]
 *   y, dy         float [T'][B][F' * C]  T' = ceil(T / st), F' = ceil(F / sf), channel fastest
 *   lengths       int32 [B] (DEVICE)     source frames of each row;  Lb = min(max(lengths[b], 0), T)
 *   lengths_out   int32 [B] (DEVICE)     L'b = ceil(Lb / st), written by the forward launch
 *   G 1 .. 3, F 1 .. 128, C 16 | 32 | 48 | 64, kt odd 1 .. 11, kf odd 1 .. 41, st and sf 1 .. 4, F' * C <= 4096
 *   fwd:  pre[t'][b][f'][c] = bias[c] + sum_{g,i,j} w[k][c] * x[t' st + i - pt][b][g][f' sf + j - pf]
 *                              over the terms whose source frame lies in 0 .. Lb - 1 and whose source bin lies in 0 .. F - 1
 *         y[t'][b][f' C + c] = min(max(pre, 0), 20) for t' < L'b,  0 for t' >= L'b
 *   bwd:  mask = 0 < y < 20 (read from y itself: no pre-activation is kept)
 *         dw[k][c] += sum_{b, t' < L'b, f'} patch_k(t', b, f') * dy * mask      db[c] += sum dy * mask      (both ACCUMULATE, as
 *         amdspeech_linear_bwd does)
 * The arithmetic is a matrix product on v_mfma_f32_16x16x4_f32, exact f32: every pre is one f32 accumulation chain over the k_pad
 * products in ascending k (terms outside the row or the band take part as exact zeros; K is padded to a multiple of 4 with zero
 * weights), then one add of the bias.  dw and db are summed in three fixed stages: per partial one chain over at most `dw_terms`
 * output positions (tiles in index order t'-tile * B + b, positions in order inside a tile); per element `reduce_slices` plain sums
 * over contiguous runs of at most `reduce_terms` partials; the slices in slice order and one add into the output.  No
 * floating-point atomics: y, dw and db are bit-identical from run to run.
 * y is written in EVERY element; frames of x at or past Lb and frames of y / dy at or past L'b are never read and may hold anything
 * (NaN included).  The workspace is written in every word the second stage reads: it needs no fill.  Asynchronous on `stream`;
 * nothing is copied to the host.  One launch forward, two backward.
 * AMDSPEECH_EINVAL with a message and no launch: null pointers (workspace included), sizes outside the ranges above, T * B * G * F or
 * T' * B * F' * C >= 2^31, B > 65535, x / y ranges that overlap (fwd), dw / db / workspace ranges that overlap (bwd).
 * amdspeech_conv2d_bwd_workspace_bytes: bytes of `ws` (device, caller-allocated, 4-byte aligned); 0 for a shape the calls refuse.
 * The figure covers the shape and every SHORTER T at the same other sizes: dw_partials only grows with T.
 * amdspeech_conv2d_plan: the launch geometry as plain numbers, a READ-ONLY view of the plan the launches themselves read (one
 * function decides for all of them); no device is needed, the shape is checked as the calls check it.
 *   t_out, f_out       T', F'
 *   k, k_pad           K and K rounded up to the instruction's k of 4 (zero weights)
 *   tile_t, tile_f     output frames and bins of one tile: tile_f = F' (all bins), tile_t = floor(128 / F'), fewer where the source
 *                      span of the tile, ((tile_t - 1) st + kt) * G * (F + 2 pf) words, would not fit LDS beside the other tenants
 *                      of either pass.  Independent of T and B.  A tile is one row b
 *   vec                words per global access (1: there is no vector path, any 4-byte aligned base takes the same kernels)
 *   fwd_workgroups     ceil(T' / tile_t) * B, 256 threads each;   fwd_lds_bytes: patch + k offsets + the weight chunk
 *   weights_resident   1: the whole [k_pad][C] passes through LDS once per workgroup (k_chunk = k_pad); 0: streamed from L2 in chunks
 *                      of k_chunk = 64 rows
 *   k_rows, k_groups   rows of a partial tile, K + 1 (the bias row) rounded up to 16, and workgroups along them (256 rows each)
 *   dw_partials        partial tiles = min(tiles, ceil(512 / k_groups));   bwd_workgroups = dw_partials * k_groups
 *   bwd_lds_bytes      patch + position offsets + dy * mask of one tile
 *   dw_terms           output positions summed into one partial: ceil(tiles / dw_partials) * tile_t * F'
 *   reduce_slices      threads per element in the second stage (8);   reduce_terms = ceil(dw_partials / 8)
 *   reduce_workgroups  of 256 threads: ceil((K + 1) * C / 32)                                                                     */
typedef struct amdspeech_conv2d_plan_info {
    int t_out, f_out, k, k_pad, tile_t, tile_f, vec, fwd_workgroups, fwd_lds_bytes, weights_resident, k_chunk, k_rows, k_groups,
        dw_partials, bwd_workgroups, bwd_lds_bytes, dw_terms, reduce_slices, reduce_terms, reduce_workgroups;
} amdspeech_conv2d_plan_info;
int amdspeech_conv2d_fwd(void* stream, const float* x, const float* w, const float* bias, const int* lengths, int T, int B, int G, int F,
                         int C, int kt, int kf, int st, int sf, float* y, int* lengths_out);
size_t amdspeech_conv2d_bwd_workspace_bytes(int T, int B, int G, int F, int C, int kt, int kf, int st, int sf);
int amdspeech_conv2d_bwd(void* stream, const float* x, const float* y, const float* dy, const int* lengths, int T, int B, int G, int F,
                         int C, int kt, int kf, int st, int sf, float* dw, float* db, void* ws);
int amdspeech_conv2d_plan(int T, int B, int G, int F, int C, int kt, int kf, int st, int sf, amdspeech_conv2d_plan_info* out);

/* ------------------------------------------- voice activity / long recordings ---
 * What cuts a recording LONGER than the model's input at its pauses (no reference counterpart: an opt-in deviation, config key
 * long_audio; nothing of it is called at the key's default): frame energies of raw PCM, speech flags from an adaptive threshold,
 * and the gather of sample spans of a long row into the padded block the resampler and the front end take.  The cut planner that
 * sits between the flags and the gather is host code (segmenter.py).  Plain launches; no kernel waits for another workgroup.
 *   pcm        float [B][n_max]     mono samples at the FILE's rate; words at or past n_samples[b] are never read
 *   n_samples  int32 [B] (HOST)     valid samples per row, 0 .. n_max
 *   hop        samples per block, >= 1 (callers pass 10 ms: round-half-even(0.01 rate)); F = ceil(n / hop) frames per row
 * amdspeech_vad_num_frames: ceil(n_samples / hop), 0 for 0 samples; host arithmetic (AMDSPEECH_EINVAL for a negative count or hop < 1).
 *
 * amdspeech_vad_energy -- energy_db float [B][f_max], f_max >= ceil(n_max / hop).  The arithmetic, per row:
 *   S[t]  = sum of double(x_i)^2 over i in [t hop, min(n, (t + 1) hop))     float64; S[t] = 0 for t >= F
 *   mean  = (S[t] + S[t + 1]) / (2 hop)            frame t covers two blocks; the divisor stays 2 hop at the ragged end
 *   energy_db[t] = float(10 log10(max(mean, 1e-12)))   for t < F;   -120 where mean is not finite (an Inf or NaN sample: the
 *   value of digital silence), and -120 in every word at t >= F up to f_max
 * The order of the sum inside a block is fixed (16 lanes stride over the block's samples, or its 16-byte vectors, and meet in an
 * 8-4-2-1 butterfly): no atomics, two calls give the same bits.  The error against a float64 evaluation is that of a float64 sum of
 * up to 2 hop exact squares, 2 hop 2^-53 relative, and of one float64 log10 rounded to float.  `ws` is not read by this call (it
 * is the workspace of the flags call, accepted so that one buffer serves both) and may be NULL.
 *
 * amdspeech_vad_flags -- speech uint8 [B][f_max], stats float [B][3] = (floor, peak, threshold), from energy_db [B][f_max] and
 * n_frames int32 [B] (HOST; 0 .. f_max).  Every operation is one float32 operation or integer logic; per row, F = n_frames[b]:
 *   k     = ((F - 1) percentile) / 100                  integer division
 *   floor = the k-th smallest (0-based) of energy_db[0 .. F), EXACT (a radix select over the order-preserving uint32 image of the
 *           floats, four 8-bit passes, counters in LDS);   peak = the largest.   energy_db must hold no NaN (the energy call writes none)
 *   thr   = min(max(floor + margin_db, peak - range_db), peak - margin_db)
 *   raw[t]    = energy_db[t] > thr && energy_db[t] > min_db
 *   open[t]   = raw[t] and the run of ones around t is at least min_run long       (runs of min_run or more survive unchanged)
 *   speech[t] = OR of open[max(t - hangover, 0) .. min(t + hangover, F - 1)];      0 for t >= F up to f_max
 * The cap peak - margin_db makes a stationary row all speech (floor + margin_db alone would make it all silence); the gate min_db
 * makes digital silence no speech.  A row with F = 0 gets stats (-120, -120, -120).
 *   ws   device, at least B * f_max * 4 bytes, 4-byte aligned -- amdspeech_vad_workspace_bytes(B, n_max, hop) for f_max =
 *        ceil(n_max / hop) (0 for a bad shape); caller-allocated.  One int per frame: the last frame at or before it that is the
 *        min_run-th or later of its run
 *
 * amdspeech_gather_spans -- out float [S][w_out] (16-byte aligned) from spans (row[s], start[s], count[s]), int32 [S] each (HOST):
 *   out[s][i] = pcm[row[s]][start[s] + i]   for i < min(count[s], n_samples[row[s]] - start[s], w_out),   0 from there up to w_out
 * A span that reaches past its row (or starts past it) yields zeros there and never reads past the row.  ONE launch for all spans;
 * 16-byte stores throughout, 16-byte loads where start[s] + i and the row base are multiples of four words.  S = 0 launches nothing
 * and succeeds.  Up to 256 spans travel as kernel arguments; more go through a device buffer of the call's own, and the call then
 * waits for the stream before it returns.  The lengths of the first two calls travel the same way (256 rows).
 *
 * AMDSPEECH_EINVAL with a message: hop < 1, percentile outside 0 .. 100, min_run < 1, hangover outside 0 .. 1024, a margin_db,
 * range_db or min_db that is NaN or infinite, a count, start or length that is negative or beyond its bound, null pointers (but
 * for `ws` of the energy call and the span arrays at S = 0), f_max < ceil(n_max / hop), B * f_max >= 2^31, w_out < 1, and a
 * pcm that is not 16-byte aligned when the plan takes 16-byte loads: such a base is REFUSED, not run with single-word accesses.
 * amdspeech_vad_plan: the launch geometry as plain numbers, a READ-ONLY view of the plan the energy call itself reads; host only.
 *   load_vec         words per load of the energy kernel: 4 when hop % 4 == 0 and (B == 1 or n_max % 4 == 0) -- every block start
 *                    is then 16-byte aligned -- else 1 (hop 441, 44.1 kHz: every second block start is odd)
 *   frames_per_tile  63: a workgroup forms 64 block sums (16 teams of 16 lanes, four rounds) and the 63 frames between them
 *   tiles_per_row, workgroups, threads   ceil(f_max / 63); tiles_per_row * min(B, 65535); 256.  The grid runs over (tile, row): one
 *                    row of an hour at 16 kHz is 5715 workgroups
 *   f_max            ceil(n_max / hop)
 *   select_passes    4: the 8-bit passes of the radix select
 *   row_workgroups, row_threads   the select and the flags kernel: min(B, 65535) workgroups of 1024 threads, one row each
 *   meta_by_copy     1 when B > 256                                                                                          */
typedef struct amdspeech_vad_plan_info {
    int load_vec, frames_per_tile, tiles_per_row, workgroups, threads, f_max, select_passes, row_workgroups, row_threads, meta_by_copy;
} amdspeech_vad_plan_info;
int amdspeech_vad_num_frames(int n_samples, int hop);
size_t amdspeech_vad_workspace_bytes(int B, int n_max, int hop);
int amdspeech_vad_plan(int B, int n_max, int hop, amdspeech_vad_plan_info* out);
int amdspeech_vad_energy(void* stream, const float* pcm, const int* n_samples, int B, int n_max, int hop,
                         float* energy_db, int f_max, void* ws);
int amdspeech_vad_flags(void* stream, const float* energy_db, const int* n_frames, int B, int f_max,
                        int percentile, float margin_db, float range_db, float min_db, int min_run, int hangover,
                        unsigned char* speech, float* stats, void* ws);
int amdspeech_gather_spans(void* stream, const float* pcm, const int* n_samples, int B, int n_max,
                           const int* row, const int* start, const int* count, int S, float* out, int w_out);

/* ------------------------------------------------------------- profiling ----
 * Optional HIP-event timing of the recurrence kernels (no reference counterpart;
 * feeds bench.py's roofline line).  When enabled, lstm_fwd / lstm_bwd bracket
 * their recurrence kernel launches (and only those: the GEMMs of the per-layer
 * H = 1024 path are left out) with hipEvents on the caller's stream.
 * amdspeech_profile_get synchronises on the last recorded pairs and returns the
 * elapsed milliseconds and the number of TIME STEPS they covered: T + L - 1
 * diagonals for a whole-stack kernel or launch chain, T * L for the per-layer
 * kernels.  which: 0 = forward, 1 = backward.                                  */
int amdspeech_profile_enable(int on);
int amdspeech_profile_get(int which, float* elapsed_ms, int* time_steps);
/* Algorithmic FLOPs (2 per multiply-add) of the last whole-sequence dataflow launch of that direction, as the library itself
 * split the work: the recurrence's own products ([B,4H]x[4H,H]: L recurrent + L-1 "down" per frame, + dZ_0 when the bottom
 * layer's groups form it; forward: L x [B,2H]x[2H,4H]) and the other products computed INSIDE the same launch (the
 * weight-gradient share of the in-kernel GEMM workers).  Zeros when the last call took another kernel family.           */
int amdspeech_profile_get_flops(int which, double* recurrence_flops, double* other_flops);

/* -------------------------------------------------- data-parallel exchange ----
 * The reference trains on one device and reaches larger batches by ACCUMULATING
 * the gradients of `mini_batch_size` mini-batches before one clip + Adam
 * (models/AcousticModel.py:391-406, driver :916-926).  N data-parallel ranks
 * with one mini-batch each are that accumulation with N = mini_batch_size: every
 * rank sums its own utterances' gradients into its flat buffer, ONE fp32 SUM
 * all-reduce over RCCL (xGMI) makes every buffer the global sum, and every rank
 * applies the identical amdspeech_clip_adam.  No TensorFlow call is replaced:
 * the reference has no multi-device path.
 *
 * Bootstrap: rank 0 calls amdspeech_comm_unique_id and hands the
 * AMDSPEECH_COMM_ID_BYTES to every rank by any host-side means (torch.distributed
 * gloo broadcast, a file, MPI ...); every rank then calls amdspeech_comm_init
 * with its device current (hipSetDevice).  RCCL is bound with dlopen at the
 * first call -- AMDSPEECH_EUNSUPPORTED when no librccl.so can be found.
 * The collectives are enqueued on `stream`, in place; `n` floats.             */
#define AMDSPEECH_COMM_ID_BYTES 128
/* AMDSPEECH_OK when this process can bind RCCL (dlopen + the symbols the collectives need), an error code otherwise: what ranks
 * other than 0 probe with before anybody enters amdspeech_comm_init -- no id, no socket, no thread is created.                */
int amdspeech_comm_available(void);
int amdspeech_comm_unique_id(void* id_out);
int amdspeech_comm_init(const void* id, int rank, int world, void** comm_out);
int amdspeech_comm_destroy(void* comm);
/* What the communicator itself reports (ncclCommUserRank / ncclCommCount / ncclGetVersion) and the path of the RCCL shared
 * object that was bound -- diagnostics for a multi-GPU run (bench.py --gpus N prints them); any out pointer may be NULL.    */
int amdspeech_comm_info(void* comm, int* rank, int* world, int* rccl_version, char* lib_path, int lib_path_len);
int amdspeech_allreduce_sum_f32(void* comm, void* stream, float* buf, long n);
int amdspeech_broadcast_f32(void* comm, void* stream, float* buf, long n, int root);

/* ------------------------------------------------------ bidirectional glue ----
 * out[t,b,:] = in[len_b-1-t, b, :] for t < len_b, 0 beyond; time-major [T,B,H],
 * H a multiple of 4; accumulate != 0 adds into out.  The tf.reverse_sequence a
 * tf.nn.bidirectional_dynamic_rnn wraps around its backward-direction cells (the
 * reference builds a unidirectional dynamic_rnn, models/AcousticModel.py:276-278;
 * BASELINE.json configs[4] asks for the bidirectional variant).  Self-adjoint:
 * the same call reverses the gradients.                                        */
int amdspeech_reverse_sequences(void* stream, const float* in, float* out, const int* lengths,
                                int T, int B, int H, int accumulate);

/* ------------------------------------------------------------------ misc ----
 * y[i] += x[i] (gradient accumulation helper), y[i] = 0.                      */
int amdspeech_axpy(void* stream, float a, const float* x, float* y, long n);
int amdspeech_fill(void* stream, float* y, float value, long n);

/* -------------------------------------------------------- language model ----
 * The two ends of a next-token language-model step over the acoustic model's label alphabet (lm.hip): the token
 * lookup in front of the LSTM stack and the softmax cross-entropy behind the output Linear.  The reference's LanguageModel feeds
 * one-hot rows through the input Linear (models/LanguageModel.py) -- the lookup below IS that product for a one-hot row -- and
 * trains with CTC on shifted labels; the cross-entropy is this build's deviation.
 *
 * All pointers are DEVICE memory; the calls are stream-ordered, do not synchronise and do not allocate.  Token arrays are
 * int32 [B][ld] row-major with ld >= T: position (t, b) reads element b * ld + t, so one buffer serves the inputs (tok) and the
 * targets (tok + 1).  lengths int32 [B]; a position is inside its row when t < lengths[b].
 *
 * amdspeech_embed_fwd: out[t][b][:] = w[id][:] + bias where t < lengths[b] and 0 <= id < V, and bias elsewhere (the zero one-hot
 *   row); w [V][H], bias [H] or NULL, out [T][B][H]; H a multiple of 4, w / bias / out 16-byte aligned.
 * amdspeech_embed_bwd: ACCUMULATES like amdspeech_linear_bwd: dw[v][:] += the sum of dz[t][b][:] over the positions inside their
 *   row that hold v; dbias[:] (may be NULL) += the sum over all positions inside their row.  No floating-point atomics: the order
 *   of every sum is a fixed function of the arguments (two runs give the same bits), and a row of dw whose token does not occur
 *   is not written.  ws: amdspeech_embed_bwd_workspace_bytes (0 for a bad shape), 16-byte aligned.
 * amdspeech_xent_fwd_bwd: logits [T][B][C], 2 <= C <= 4096.  A position is live when t < lengths[b] and 0 <= target < C; there
 *   nll = logsumexp(row) - row[target] (with the row maximum subtracted) and dlogits = scale * (softmax(row) - onehot(target));
 *   every other position gets nll = 0 and a zero dlogits row.  loss[b] is the float32 rounding of the float64 sum, in increasing
 *   t, of the float32 nll[t][b].  nll [T][B] may be NULL; dlogits may be NULL (the scoring call) or BE logits (a row is read
 *   completely before it is written).  ws: amdspeech_xent_workspace_bytes (0 for a bad shape).
 * amdspeech_xent_plan: the row kernel and launch geometry of a shape as plain numbers, a READ-ONLY view of the plan the launch
 *   itself reads (one function decides for both); no device is needed and nothing is launched.  c_min .. c_max is the range of C
 *   that takes the very same kernel instantiation: the tests walk the boundaries from it.                                    */
#define AMDSPEECH_XENT_KERNEL_WAVE 0  /* one wavefront per row, values_per_lane logits in each lane's registers (C <= 1024) */
#define AMDSPEECH_XENT_KERNEL_BLOCK 1 /* one 256-thread workgroup per row, the row maximum and sum across its four waves through LDS */
typedef struct amdspeech_xent_plan_info {
    int kernel, values_per_lane, threads, rows_per_workgroup, grid, c_min, c_max, loss_threads, loss_grid;
} amdspeech_xent_plan_info;
int amdspeech_embed_fwd(void* stream, const int* ids, int ld, const int* lengths, int T, int B, int V, int H,
                        const float* w, const float* bias, float* out);
size_t amdspeech_embed_bwd_workspace_bytes(int T, int B, int V, int H);
int amdspeech_embed_bwd(void* stream, const int* ids, int ld, const int* lengths, int T, int B, int V, int H,
                        const float* dz, float* dw, float* dbias, void* ws);
size_t amdspeech_xent_workspace_bytes(int T, int B, int C);
int amdspeech_xent_plan(int T, int B, int C, amdspeech_xent_plan_info* out);
int amdspeech_xent_fwd_bwd(void* stream, const float* logits, const int* targets, int ld, const int* lengths, int T, int B,
                           int C, float scale, float* nll, float* loss, float* dlogits, void* ws);

/* amdspeech_lm_step (lm_step.hip): ONE step of the language model for N hypotheses, each from its own parent state,
 * gathered from a state pool -- what a beam search with the model inside it needs (amdspeech_ctc_beam_search_host_fused below).
 * The pool is two f32 device arrays pool_h, pool_c of shape [n_slots][L][H] (amdspeech_lm_step_pool_bytes: the bytes of ONE of
 * them, 0 for a bad shape).  parent / token / dest: device int32 [N].  Per row r, exactly f32 whatever precision trained the model:
 *     x_0 = input_w[token[r]] + input_b                      (the bias alone for a token outside 0 .. V-1, as amdspeech_embed_fwd)
 *     g = [x_l ; h_parent,l] . kernel_l + bias_l             (BasicLSTMCell: gates i, j, f, o; forget bias 1.0; no dropout)
 *     c' = c_parent s(f + 1) + s(i) tanh(j),  h' = s(o) tanh(c'),  x_{l+1} = h'     -> slot dest[r], layer l
 *     logq[r][:] = log_softmax(h'_top . output_w + output_b)  natural log, the row maximum subtracted; logq device [N][V]
 * parent[r] == -1 is the zero state (the start of a sentence).  kernel_l = kernel_0 + l * kernel_stride ([2H][4H]), bias_l =
 * bias_0 + l * bias_stride (floats), as the LSTM calls take them.
 *   - dest entries must be distinct and no dest slot may also be a parent slot of the same call; the C call does NOT check this
 *     (the indices are on the device).  An index outside its range touches nothing outside the buffers: a parent outside
 *     -1 .. n_slots-1 reads the zero state, a row whose dest is outside 0 .. n_slots-1 is not written (its logq row neither).
 *   - Slots not named in dest keep their bits.
 *   - A row's h', c', logq depend on that row's parent state, token and the weights ONLY -- not on N, the row's position or the
 *     other rows, bit for bit: every instantiation contracts k in the same fixed order and there are no atomics.
 *   - L + 1 plain launches (one per layer, one for the output layer and log-softmax); no workgroup waits for another one.  The gate
 *     pre-activations stay on the chip, the parent rows are gathered through the index while the operands are loaded.
 *   - H a multiple of 16 in 16 .. 4096, 2 <= V <= 256, 1 <= L <= 8, 1 <= N < 2^24, n_slots >= 1 with n_slots * L * H < 2^31;
 *     pointers 16-byte aligned, kernel_stride / bias_stride multiples of 4 floats: otherwise AMDSPEECH_EINVAL (a bad argument) or
 *     AMDSPEECH_EUNSUPPORTED (a size limit of the kernels) with a message that names the limit, and nothing is launched.
 * amdspeech_lm_step_plan: the instantiation and launch geometry of a shape, a READ-ONLY view of the plan the launch itself reads;
 *   no device is needed.  n_min .. n_max is the range of N that takes the very same instantiation (row_tile = 16 or 32 rows per
 *   workgroup).                                                                                                                   */
#define AMDSPEECH_LM_STEP_KERNEL_MFMA16 0 /* v_mfma_f32_16x16x4_f32, the rows on the A port, k split over the four waves of a workgroup */
typedef struct amdspeech_lm_step_plan_info {
    int kernel, row_tile, threads, launches, n_min, n_max, col_tiles, row_tiles, lds_bytes, out_row_tile, out_row_tiles, v_max;
} amdspeech_lm_step_plan_info;
int amdspeech_lm_step(void* stream, int N, const int* parent, const int* token, const int* dest,
                      float* pool_h, float* pool_c, int n_slots, int L, int H, int V,
                      const float* input_w, const float* input_b, const float* kernel_0, long kernel_stride,
                      const float* bias_0, long bias_stride, const float* output_w, const float* output_b,
                      float* logq);
int amdspeech_lm_step_plan(int N, int L, int H, int V, amdspeech_lm_step_plan_info* out);
size_t amdspeech_lm_step_pool_bytes(int n_slots, int L, int H);

/* The prefix beam search of amdspeech_ctc_beam_search_host_nbest with the language model INSIDE the beam (first-pass fusion).
 * HOST pointers.  `step` advances the model: for n new hypotheses it gets parent[k] (a state slot, -1 = the start of a sentence),
 * token[k] and dest[k] (the slot that receives the new state) and fills logq [n][C], the model's natural-log next-token
 * distribution after that token; a non-zero return ends the search with that status and no further callback.  `step` is only
 * ever called on the calling thread, once per frame for ALL utterances of the mini-batch (at most T + 1 calls), the first one
 * being the root alone (parent -1, token C-1 -> dest root).  Within a call the dest slots are distinct and none is a parent.
 * Slots: utterance b owns 2 * beam_width of them and the last one is the shared root: amdspeech_ctc_beam_search_fused_slots.
 * Scoring: the extension of a beam entry by the non-blank label c adds lm_weight * q[c] + lm_length_bonus to the acoustic
 * from + lp[c], q being the model's row for the entry's prefix AS THE TRIE HOLDS IT -- before merge_repeated: "b b" is scored as
 * the model sees "b b" --, also where that extension merges into a beam child; blank and repeat transitions add nothing; after
 * the last frame an entry's score is tot + lm_weight * q[C-1] (the closing EOS).  Candidates are selected exhaustively.  The
 * outputs are those of the n-best call in (final score descending, lexicographic) order, log_prob the final score; n_best == 0
 * means one path: ids [B][T], out_len [B], log_prob [B] (may be NULL), n_found unused.                                        */
typedef int (*amdspeech_lm_step_fn)(void* user, int n, const int* parent, const int* token, const int* dest, float* logq);
int amdspeech_ctc_beam_search_fused_slots(int B, int beam_width);
int amdspeech_ctc_beam_search_host_fused(const float* logits, const int* lengths, int T, int B, int C, int beam_width,
                                         int merge_repeated, int n_best, float lm_weight, float lm_length_bonus,
                                         amdspeech_lm_step_fn step, void* user, int* ids, int* out_len, float* log_prob,
                                         int* n_found, int max_threads);

/* ------------------------------------------------- blank-frame skipping ---
 * What shortens the input of the host beam decoders above (no reference counterpart: an opt-in deviation, config key
 * decode_blank_skip; nothing of it is called at the key's default): the frames on which a CTC model is nearly sure of blank are
 * dropped before the search, per utterance and in order ("phone-synchronous decoding").  ctc_blank_skip.hip; DESIGN.md 4.7b.
 *   logits      float [T][B][C] (device)    blank is class C-1
 *   lengths     int32 [B] (device)          as amdspeech_ctc_greedy_decode takes them; n_b = min(max(lengths[b], 0), T)
 *   log_threshold  log of the blank probability above which a frame is skippable; finite and <= 0
 * Per utterance b, every operation one float32 operation:
 *   lpb[t]  = (logits[t][b][C-1] - max_c logits[t][b][c]) - log(sum_c exp(logits[t][b][c] - max))
 *   skip[t] = t < n_b && lpb[t] >= log_threshold        (a NaN lpb compares false: the frame is kept)
 *   keep[t] = t < n_b && !(skip[t] && t > 0 && skip[t-1])
 * The run rule: of every maximal run of skippable frames the FIRST is kept and the rest are dropped.  A repeated label on both
 * sides of a blank run then still has a blank frame between its two spikes, so merge_repeated and the prefix beam's "a repeat
 * starts a new character only after a blank" rule see what they saw before; dropping whole runs would merge "a _ a" into "a".
 * Outputs, with j = 0 .. n'_b - 1 walking the kept frames of b in increasing t:
 *   out_logits  float [T][B][C]   out_logits[j][b][:] = logits[t_j][b][:], copied bit for bit; every other word is written as 0
 *   out_lengths int32 [B]         n'_b
 *   src_frame   int32 [B][T]      src_frame[b][j] = t_j; every other word is written as -1
 *   blank_logp  float [T][B] or NULL   the stage quantity lpb[t] for t < n_b, 0 elsewhere (for the tests)
 * The maximum and the sum of a row are taken in an order that is a fixed function of C (lane l of a wavefront, or of a 256-thread
 * workgroup above 1024 classes, adds its own words in increasing c, the lanes meet in a 32-16-8-4-2-1 xor butterfly, the four
 * waves of a workgroup in wave order): no floating-point atomics, two calls give the same bits, and a row's outputs depend only on
 * that row's own frames and length -- not on B or on the row's position.  |lpb - exact| <= u (6 M + C + 5 ln C + 4) to first order,
 * u = 2^-24, M the largest |logit| of the frame.  A frame at or past n_b is not read.
 * The call is stream-ordered, does not synchronise on the host and does not allocate: three plain launches (rows, scan, gather).
 *   ws   device, amdspeech_ctc_blank_skip_workspace_bytes(T, B, C) bytes (0 for a bad shape): one flag byte per frame
 * out_logits must not overlap logits (rows move forward in time): such a call is refused.  Limits: 2 <= C <= 4096, T >= 1, B >= 1,
 * T * B * C < 2^31; logits and out_logits 16-byte aligned when C % 4 == 0.  AMDSPEECH_EINVAL (a bad argument: T, B or C below its
 * minimum, a log_threshold that is NaN, infinite or above 0, a null pointer but for blank_logp, overlap, alignment) or
 * AMDSPEECH_EUNSUPPORTED (a size limit of the kernels: C > 4096, T * B * C >= 2^31) with a message that names the limit, and
 * nothing is launched.
 * amdspeech_ctc_blank_skip_plan: the kernels and launch geometry of a shape as plain numbers, a READ-ONLY view of the plan the
 * launch itself reads (one function decides for both); no device is needed and nothing is launched.
 *   kernel, words_per_lane, vec   the row kernel, the words of a row each lane holds (4, 8, 16 | 8, 16) and how it loads them: 4 = 16-byte
 *                    vectors (C % 4 == 0), 1 = single words.  The gather copies with the same width
 *   c_min .. c_max   the range of C with the same kernel and words_per_lane: the tests walk the boundaries from it
 *   rows_threads, rows_per_workgroup, rows_grid   256; 4 (wave) or 1 (block); ceil(T B / rows_per_workgroup)
 *   t_chunk, chunks  256 frames per step of the per-utterance scan, one per thread, the count of kept frames carried; ceil(T / 256)
 *   scan_threads, scan_grid       256; B
 *   gather_threads, gather_grid   256; ceil(T B C / vec / 256)
 *   launches, workspace_bytes     3; T B rounded up to 256                                                                     */
#define AMDSPEECH_BLANK_SKIP_KERNEL_WAVE 0  /* one wavefront per row, words_per_lane logits in each lane's registers (C <= 1024) */
#define AMDSPEECH_BLANK_SKIP_KERNEL_BLOCK 1 /* one 256-thread workgroup per row, the maximum and the sum across its four waves through LDS */
typedef struct amdspeech_ctc_blank_skip_plan_info {
    int kernel, words_per_lane, vec, c_min, c_max, rows_threads, rows_per_workgroup, rows_grid, t_chunk, chunks, scan_threads, scan_grid,
        gather_threads, gather_grid, launches, workspace_bytes;
} amdspeech_ctc_blank_skip_plan_info;
size_t amdspeech_ctc_blank_skip_workspace_bytes(int T, int B, int C);
int amdspeech_ctc_blank_skip_plan(int T, int B, int C, amdspeech_ctc_blank_skip_plan_info* out);
int amdspeech_ctc_blank_skip(void* stream, const float* logits, const int* lengths, int T, int B, int C, float log_threshold,
                             float* out_logits, int* out_lengths, int* src_frame, float* blank_logp, void* ws);

/* ------------------------------------------------------------ transducer ---
 * The transducer (RNN-T) objective: label preparation, the joint network forward and backward, and the lattice loss with its
 * gradient (no reference counterpart: an opt-in deviation; nothing of it is called by a CTC model).  transducer.hip; DESIGN.md 4.10.
 * All pointers are device memory; the calls are stream-ordered, do not synchronise, do not allocate and use no floating-point
 * atomics: two runs give the same bits.  Every offset into a lattice tensor is computed in 64 bits.
 *   f        float [T][B][J]       the encoder projection, time-major
 *   g        float [U+1][B][J]     the prediction projection, time-major
 *   w_out    float [J][C], b_out float [C]
 *   lattice tensors (logits, dlogits)   float [B][T][U+1][C]
 *   lengths  int32 [B]; T_b = min(max(lengths[b], 0), T).   n int32 [B]: the target count n_b of row b (clamped to 0 .. U).
 * Blank is class C-1.  Node (b, t, u) is LIVE when t < T_b and u <= n_b.
 * Limits, the same for every call: J a multiple of 16 in 16 .. 1024, 2 <= C <= 256, 1 <= U <= 2559, T >= 1, B >= 1,
 * B T (U+1) C < 2^31.  Anything else is AMDSPEECH_EINVAL (a bad argument) or AMDSPEECH_EUNSUPPORTED (a size limit of the
 * kernels: J > 1024, C > 256, U > 2559, the product) with a message that names the limit, and nothing is launched.
 *
 * amdspeech_rnnt_targets: the label sparsification of amdspeech_ctc_loss_fwd_bwd on dense_labels [B][U] -- zeros are dropped, the
 *   target is every kept label before the first one >= C-1 -- WITHOUT its empty-row and required-time rules: an empty target is
 *   n_b = 0, a valid row.  Negative ids are dropped with the zeros (every target is a class in 1 .. C-2: ln P is finite).  Writes targets [B][U] (0 past n_b), n [B], the prediction network's token rows tok [B][U+2] =
 *   [C-1, y_1 .. y_n, C-1, ...] (the start symbol is the EOS id, as the language model has it) and tok_len [B] = n_b + 1.
 * amdspeech_rnnt_joint_fwd: logits[b,t,u,:] = tanh(f[t,b,:] + g[u,b,:]) . w_out + b_out on every live node, exact f32 on
 *   v_mfma_f32_16x16x4_f32.  z = tanh(.) is formed in registers from LDS strips of f and g and is never written to memory.  The k
 *   order of a node's sum is a fixed function of J, so a node's bits do not depend on B, T, U or its neighbours.  Dead nodes are
 *   not written; nothing downstream reads them.
 * amdspeech_rnnt_loss_fwd_bwd: row log-softmax in float32 (the row maximum subtracted), alpha and beta over the lattice in log
 *   space with a float64 state, walked by anti-diagonals, the two walks of an utterance concurrently;
 *     loss[b] = -ln P = -(alpha(T_b-1, n_b) + lp_blank(T_b-1, n_b)),
 *     dlogits[b,t,u,v] = p_v gamma - [v = C-1] exp(alpha + lp_blank + beta(t+1,u) - ln P) - [v = y_{u+1}, u < n_b] exp(alpha +
 *     lp_y + beta(t,u+1) - ln P),   gamma = exp(alpha + beta - ln P) at (t,u), beta past the terminal node 0
 *   = d(sum_b loss_b)/dlogits.  dlogits may BE logits (a row is read completely before it is written).  Dead nodes get zero rows;
 *   a row with T_b = 0 gets loss 0 and no gradient.  ws: amdspeech_rnnt_workspace_bytes (any valid J), 256-byte aligned.
 * amdspeech_rnnt_joint_bwd: with dz = (dlogits . w_out^T) (1 - z^2), z recomputed on the chip:  dw_out += z^T . dlogits,
 *   db_out += sum dlogits (accumulated, as amdspeech_linear_bwd),  df[t,b,:] = sum_u dz,  dg[u,b,:] = sum_t dz (overwritten; rows
 *   without a live node are zero).  Neither z nor dz is written to memory: df is complete inside a workgroup, dg leaves one
 *   partial per chunk of frames and dw_out / db_out one per workgroup, added by a second pass in a fixed order.  Reads the dlogits
 *   of live nodes only.  ws: the same workspace.
 * amdspeech_rnnt_workspace_bytes (0 for a bad shape), with N = B T (U+1) and every region rounded up to 256 bytes:
 *     4 N + 4 N (blank / label log-probabilities) + 8 N + 8 N (alpha, beta) + 8 B (ln P)
 *     + 4 bwd_t_chunks (U+1) B J (dg partials) + 4 bwd_items J C + 4 bwd_items C (dw_out / db_out partials)
 *   -- bwd_t_chunks = ceil(T / bwd_t_chunk) is at most 8 up to T = 1024 (no term grows with N J there); beyond, bwd_t_chunk stays
 *   128 frames and the dg partials are N J / 128 words.
 * amdspeech_rnnt_plan: a READ-ONLY view of the plan the launches themselves read (one function decides for both); no device is
 *   needed and nothing is launched.
 *   threads                      256, every joint and row kernel
 *   col_tiles, c_min .. c_max    column tiles of 16 classes of the joint kernels, and the range of C with the same instantiation
 *   j_min .. j_max               the range of J with the same instantiation (J is a loop count: all of it)
 *   fwd_t_tile, fwd_u_tile, fwd_k_chunk   joint_fwd: 4 frames (one per wave) x 16 / 32 / 64 prefix positions per workgroup, 32 k per
 *                                LDS chunk;  fwd_t_tiles, fwd_u_tiles, fwd_grid = their product times B;  fwd_lds_bytes
 *   rows_per_workgroup, rows_grid   the log-probability and gradient kernels: one wavefront per node
 *   rec_kernel, rec_threads, rec_states, u_min .. u_max   the recursion kernel (AMDSPEECH_RNNT_REC_* below), its threads per
 *                                (utterance, direction), the lattice columns a thread holds, and the range of U on that kernel;
 *                                rec_grid = 2 B;  rec_lds_bytes
 *   bwd_t_tile, bwd_u_tile       joint_bwd: 4 frames (one per wave) x 16 prefix positions per step
 *   bwd_k_slice, bwd_k_slices    the slice of J a workgroup owns (64 / 32 / 16) and their number
 *   bwd_t_chunk, bwd_t_chunks    frames per workgroup (32 .. 128) and the chunks of T;  bwd_items = B bwd_t_chunks;
 *                                bwd_grid = bwd_items bwd_k_slices;  bwd_lds_bytes
 *   dg_terms, dw_terms           partials the second pass adds per element;  reduce_dg_grid, reduce_dw_grid
 *   launches_fwd, launches_loss, launches_bwd   1, 3, 3                                                                        */
#define AMDSPEECH_RNNT_REC_WAVE 0    /* one wavefront per (utterance, direction): U <= 63 */
#define AMDSPEECH_RNNT_REC_BLOCK1 1  /* 256 threads, one lattice column each: U <= 255 */
#define AMDSPEECH_RNNT_REC_BLOCK4 2  /* 256 threads, four columns each: U <= 1023 */
#define AMDSPEECH_RNNT_REC_BLOCK10 3 /* 256 threads, ten columns each: U <= 2559 */
typedef struct amdspeech_rnnt_plan_info {
    int threads, col_tiles, c_min, c_max, j_min, j_max, fwd_t_tile, fwd_u_tile, fwd_k_chunk, fwd_t_tiles, fwd_u_tiles, fwd_grid,
        fwd_lds_bytes, rows_per_workgroup, rows_grid, rec_kernel, rec_threads, rec_states, u_min, u_max, rec_grid, rec_lds_bytes,
        bwd_t_tile, bwd_u_tile, bwd_k_slice, bwd_k_slices, bwd_t_chunk, bwd_t_chunks, bwd_items, bwd_grid, bwd_lds_bytes, dg_terms,
        dw_terms, reduce_dg_grid, reduce_dw_grid, launches_fwd, launches_loss, launches_bwd;
} amdspeech_rnnt_plan_info;
int amdspeech_rnnt_plan(int T, int B, int U, int J, int C, amdspeech_rnnt_plan_info* out);
size_t amdspeech_rnnt_workspace_bytes(int T, int B, int U, int J, int C);
int amdspeech_rnnt_targets(void* stream, const int* dense_labels, int B, int U, int C, int* targets, int* n, int* tok,
                           int* tok_len);
int amdspeech_rnnt_joint_fwd(void* stream, const float* f, const float* g, const float* w_out, const float* b_out,
                             const int* lengths, const int* n, int T, int B, int U, int J, int C, float* logits);
int amdspeech_rnnt_loss_fwd_bwd(void* stream, const float* logits, const int* targets, const int* n, const int* lengths,
                                int T, int B, int U, int C, float* loss, float* dlogits, void* ws);
int amdspeech_rnnt_joint_bwd(void* stream, const float* dlogits, const float* f, const float* g, const float* w_out,
                             const int* lengths, const int* n, int T, int B, int U, int J, int C, float* df, float* dg,
                             float* dw_out, float* db_out, void* ws);
/* The L layer launches of amdspeech_lm_step without the output launch (the same code, not a copy): the same slot contract and the
 * same bits in the pool.  What a decoder calls that reads the top layer's h' itself (the transducer's prediction network).      */
int amdspeech_lm_step_state(void* stream, int N, const int* parent, const int* token, const int* dest,
                            float* pool_h, float* pool_c, int n_slots, int L, int H, int V,
                            const float* input_w, const float* input_b, const float* kernel_0, long kernel_stride,
                            const float* bias_0, long bias_stride);

/* amdspeech_rnnt_greedy_step: ONE iteration of time-synchronous greedy transducer decoding for B rows in lockstep.  Row b holds a
 * frame index t_idx[b], an emitted count m[b] and its current prediction-network slot slot[b] (2 b or 2 b + 1 of the pool
 * pool_h [2 B][L][H]), all in device arrays.  The call forms g_b = pool_h[slot_b][L-1] . w_pred + b_pred (w_pred [H][J]), the joint
 * row tanh(f[t_b, b, :] + g_b) . w_out + b_out, and its argmax over C, ties to the smallest class (every sum in increasing k).
 *   blank (C-1):  t_idx[b] += 1;  dest[b] = -1
 *   otherwise:    ids[b][m_b] = class, m[b] += 1, and (parent, token, dest)[b] = (slot_b, class, the row's other slot) for the
 *                 amdspeech_lm_step_state call that follows; slot[b] becomes dest[b]
 * A row is finished when t_b = T_b or m_b = U: a no-op that writes dest -1, and by the lm_step contract such a row is not
 * written.  The host launches T_run + U iterations (each followed by amdspeech_lm_step_state on B rows) and reads nothing in
 * between.  ids int32 [B][U].  The limits of the other transducer calls, 1 <= L <= 8, 2 B L H < 2^31.                         */
int amdspeech_rnnt_greedy_step(void* stream, const float* f, const int* lengths, int T, int B, int U, int J, int C,
                               const float* pool_h, int L, int H, const float* w_pred, const float* b_pred,
                               const float* w_out, const float* b_out, int* t_idx, int* m, int* slot, int* ids, int* parent,
                               int* token, int* dest);

#ifdef __cplusplus
}
#endif
#endif /* AMDSPEECH_H */
