"""The GEMMs per kernel variant -- exact f32, bf16x3, plain bf16 and the packed bf16 path with its operand copies: the case table, exact
references and operand placement of tests/test_cpu_gemm_ref.py and tests/test_gpu_gemm_paths.py.  A checker only: the product never
imports it.

Every case names ONE call (entry, precision, layouts, shape, strides, element offsets, bias / accumulate / column sums / count) and
the plan it was written for: the fields of ops.gemm_plan (packed: ops.gemm_bf16_packed_plan) that matter for it.
test_cpu_gemm_ref.py holds every expected plan against the query and asserts that the table reaches every (family, variant) pair the
dispatch can produce (VARIANTS below).

Three operand kinds (operands()):
  ints    every operand, the bias and the prior contents of C / colsum are integers in [-3, 3] stored as f32.  Products and their sums
          are exact in f32 in ANY order while they stay below 2^24 (9 K + 16 here), split K with f32 atomics or partial tiles
          included: the result must equal the integer product BIT FOR BIT.  One dropped, doubled or misplaced term fails.  The
          integers are exact in bf16 too (lo = 0), so the reduced-precision kernels owe the same bits.
  select  one operand is 0/1 with exactly one 1 per output row ("selA": A selects, C[m, :] = B[k(m), :]) or per output column
          ("selB": C[:, n] = A[:, k(n)]); the other is randn with full mantissas.  k() covers 0, K - 1 and both sides of every split
          boundary.  Every other term is an exact zero, so the result is the selected element AS THE ARITHMETIC CARRIES IT, bit for
          bit (arith()): all 24 bits in exact f32 (and where a reduced-precision call falls back to the f32 ladder); bf16(x) in
          plain bf16 and on the packed path; bf16(x) + bf16(x - bf16(x)) in bf16x3 -- a sum f32 holds exactly.  In bf16x3 the
          data's lo half travels through hi.lo and B's lo plane when A selects, through lo.hi and A's lo plane when B selects:
          the two probes together see each cross term and each plane.  Under accumulate: C0 + that, one f32 rounding.
  normal  randn operands against the float64 product of the f32 operands, rel_err < 2e-5 of max|ref|: the criterion of
          tests/test_gpu_kernels.py, not a new number.  Reduced precision: that file's absolute bounds, 6e-5 sqrt(K) (bf16x3) and --
          against the float64 product of the ROUNDED operands -- 2e-6 sqrt(K) (bf16, packed), times 4, or 8 under accumulate.

The copies of the packed path (entries copy, copy_t, transpose16: ops.bf16_copy, ops.bf16_transpose) have two kinds: `ints`, and
`normal` = randn across magnitudes 2^-60 .. 2^60 with +-0, exact ties to even in both directions, values next to a tie and mantissas
that carry into the next power of two planted (copy_values()).  Every copied value is compared BIT FOR BIT with
torch.Tensor.to(torch.bfloat16); fused column sums are exact for ints and judged at REL_TOL otherwise.  NaN, denormals and values that
round to infinity are left out: their handling by the copies is unpinned.

place() puts every operand into a larger buffer as a strided view: one guard row before and after, ld - width padding columns.  The
INPUTS' surroundings are NaN -- a kernel that multiplies out-of-extent bytes by a zero weight fails here and passes with the zero
padding of an ordinary test; the surroundings of C and colsum are 7.0 (bf16 destinations: the bits of bf16 7.0) and must still be
that, bit for bit, afterwards."""
import numpy as np

GROUP_MAX = 10            # AMDSPEECH_GEMM_GROUP_MAX (include/amdspeech.h)
FALLBACK_ENV = {"AMDSPEECH_GEMM_DIRECT": "0", "AMDSPEECH_GEMM_KC_DIRECT": "0"}      # everything through the LDS kernel (read once per process)
MODES = ("default", "fallback")
REL_TOL = 2e-5            # tests/test_gpu_kernels.py: rel_err of the exact-f32 GEMM
PAD_IN = float("nan")     # surroundings of the inputs
PAD_OUT = 7.0             # surroundings of the outputs


def case(name, entry, M, N, K, plan, ta=False, tb=False, lda=None, ldb=None, ldc=None, off=(0, 0, 0), bias=False, acc=False,
         colsum=False, count=1, precision=0, fallback=None, plain=False):
    """M, N, K: the PRODUCT's shape (C [M, N], K the contracted axis) whatever the entry:
         gemm        ops.gemm / gemm_bf16x3 / gemm_bf16 (by precision)
         linear_bwd  ops.linear_bwd(x [K, M], w, dy [K, N], dw [M, N], db [N], need_dx=False): trans_a, accumulate, column sums of dy
         tn_group    ops.gemm_tn_group: `count` products A_i^T . B_i; colsum=True gives column sums to the EVEN problems only
         colsum      ops.colsum_accumulate(x [K, N], out [N]): no plan (the query is about products)
         packed      ops.gemm_bf16_packed (planned by ops.gemm_bf16_packed_plan; precision 2 by definition)
         copy        ops.bf16_copy(x [K, N] (ld = ldb), dst [K, N] dense): no plan
         copy_t      ops.bf16_copy(x [K, N] (ld = ldb), dst [N, K] (ld = ldc), transpose=True, colsum [N], plain [K, N]): no plan
         transpose16 ops.bf16_transpose(x [K, N] dense bf16, dst [N, K] (ld = ldc)): no plan
       ld*: None = contiguous; off: element offset of (A, B, C) into their buffers (1 = rows not 16-byte aligned)."""
    if entry == "linear_bwd":
        ta, tb, acc, colsum = True, False, True, True
    if entry == "tn_group":
        ta, tb = True, False
    if entry == "packed":
        precision = 2
    plans = {"default": plan}
    if fallback is not None:
        plans["fallback"] = fallback
    return dict(name=name, entry=entry, M=M, N=N, K=K, ta=ta, tb=tb, lda=lda, ldb=ldb, ldc=ldc, off=off, bias=bias, acc=acc, colsum=colsum,
                count=count, precision=precision, plan=plans, plain=plain)


def P(family, variant, **kw):
    return dict(family=family, variant=variant, **kw)


LDS_TN = P("lds", 0, a_vec=1, b_vec=1)      # what the LDS-free kernels' cases take under FALLBACK_ENV
CASES = [
    # ---- gemm_skinny_n_kernel<NT>: M = 257 = four row blocks and a last wave with ONE live row
    case("skn-nt1-bias", "gemm", 257, 16, 64, P("skinny_n", 1, grid=5, splits=1, atomic=0), bias=True),
    case("skn-nt2-acc", "gemm", 257, 32, 68, P("skinny_n", 2), acc=True),
    case("skn-nt3-lda", "gemm", 257, 44, 200, P("skinny_n", 3), lda=204),
    case("skn-nt4-ldc", "gemm", 257, 64, 84, P("skinny_n", 4), ldc=68, bias=True, acc=True),
    case("skn-nt5", "gemm", 257, 68, 200, P("skinny_n", 5)),
    case("skn-nt6-ldb", "gemm", 300, 96, 84, P("skinny_n", 6), ldb=100, bias=True),
    # ---- gemm_skinny_k_kernel<KT, B_KC>: variant = KT * 2 + transB
    case("skk-kt3-nn", "gemm", 300, 64, 20, P("skinny_k", 6, col_slices=1, grid=3), bias=True),
    case("skk-kt3-nt", "gemm", 513, 68, 44, P("skinny_k", 7, col_slices=1), tb=True, acc=True),
    case("skk-kt3-nn-2slices", "gemm", 300, 256, 48, P("skinny_k", 6, col_slices=2, grid=6), bias=True, lda=52),
    case("skk-kt3-nt-2slices", "gemm", 300, 1000, 20, P("skinny_k", 7, col_slices=2), tb=True, acc=True, ldc=1004),
    case("skk-kt5-nn", "gemm", 300, 64, 52, P("skinny_k", 10, col_slices=1)),
    case("skk-kt5-nt", "gemm", 513, 68, 80, P("skinny_k", 11, col_slices=1), tb=True, bias=True, acc=True, ldb=84),
    # ---- gemm_skinny_tn_kernel<F, R>: variant = F * 8 + R; K = 4100 leaves most row chunks empty (splits * k_chunk >> K).
    #      "small is A" = M <= N; linear_bwd sums the columns of B: the WIDE operand's when small is A (a ones column: s_eff = s + 1)
    case("sktn-01", "gemm", 16, 128, 4100, P("skinny_tn", 1, atomic=1, zero_fill=1, splits=128, k_chunk=64, grid=256), ta=True),
    case("sktn-02-colsum-small", "linear_bwd", 128, 32, 4100, P("skinny_tn", 2, zero_fill=0)),
    case("sktn-03-acc", "gemm", 44, 132, 4100, P("skinny_tn", 3, zero_fill=0), ta=True, acc=True),
    case("sktn-04-colsum-wide", "linear_bwd", 60, 200, 4100, P("skinny_tn", 4)),
    case("sktn-10-small-b", "gemm", 200, 64, 4100, P("skinny_tn", 8, zero_fill=1), ta=True),
    case("sktn-11-ones-column", "linear_bwd", 64, 128, 4100, P("skinny_tn", 9)),
    case("sktn-12-lda", "gemm", 96, 128, 4100, P("skinny_tn", 10), ta=True, lda=100),
    case("sktn-13-small-b-ldc", "gemm", 132, 108, 4100, P("skinny_tn", 11), ta=True, ldc=112, acc=True),
    case("sktn-14-colsum-wide", "linear_bwd", 124, 132, 4100, P("skinny_tn", 12)),
    # ---- gemm_f32_tn_group_kernel, one problem (variant = count): through ops.gemm(trans_a=True) and, for column sums, linear_bwd
    case("tn-odd-k", "gemm", 128, 128, 33, P("tn_direct", 1, splits=1, atomic=0, zero_fill=0, map=0, grid=1), ta=True, fallback=LDS_TN),
    case("tn-split-odd-k", "gemm", 256, 256, 2051, P("tn_direct", 1, splits=8, k_chunk=258, atomic=1, zero_fill=1, map=2, bm=2, bn=2, grid=32),
         ta=True, fallback=P("lds", 0, splits=8, map=1)),
    case("tn-ragged-m-blocks", "gemm", 130, 640, 2112, P("tn_direct", 1, splits=8, k_chunk=264, map=2, bm=2, bn=5, grid=80), ta=True,
         lda=132, fallback=LDS_TN),      # (contiguous, lda = 130: rows not 16-byte aligned -- the LDS kernel with a_vec = 0)
    case("tn-odd-m-in-lda", "gemm", 257, 128, 600, P("tn_direct", 1, splits=2, k_chunk=300, map=0, grid=6, tiles_m=3), ta=True, lda=260,
         fallback=LDS_TN),
    case("tn-ragged-n-acc-one-split", "gemm", 128, 200, 200, P("tn_direct", 1, splits=1, atomic=1, zero_fill=0, map=0), ta=True, acc=True,
         ldb=204, ldc=204, fallback=LDS_TN),
    case("tn-colsum", "linear_bwd", 128, 256, 300, P("tn_direct", 1, splits=1, atomic=1), fallback=LDS_TN),
    # ---- ... and grouped, through ops.gemm_tn_group
    case("tng-2-xcd", "tn_group", 128, 512, 1024, P("tn_direct", 2, splits=4, k_chunk=256, map=1, bm=0, bn=0, grid=32, zero_fill=1), count=2),
    case("tng-2-linear-acc", "tn_group", 384, 128, 600, P("tn_direct", 2, splits=2, k_chunk=300, map=0, grid=12, zero_fill=0), count=2, acc=True,
         colsum=True),
    case("tng-2-blocks-ragged", "tn_group", 250, 500, 1030, P("tn_direct", 2, splits=4, k_chunk=258, map=2, bm=2, bn=2, grid=64), count=2,
         lda=252, colsum=True),
    case("tng-3-ragged-acc", "tn_group", 130, 132, 77, P("tn_direct", 3, splits=1, atomic=1, map=0, grid=12), count=3, acc=True, lda=132, ldc=136),
    case("tng-max", "tn_group", 128, 128, 100, P("tn_direct", GROUP_MAX, splits=1, atomic=0, map=0, grid=10), count=GROUP_MAX, colsum=True),
    # ---- gemm_f32_kc_direct_kernel<B_KC>: variant = transB
    case("kc-one-tile-8-splits", "gemm", 128, 100, 2048, P("kc_direct", 0, splits=8, k_chunk=256, map=1, grid=8, zero_fill=1), bias=True,
         fallback=P("lds", 2, splits=8)),
    case("kc-band-one-row-last", "gemm", 4100, 512, 2048, P("kc_direct", 1, splits=2, k_chunk=1024, map=3, tiles_m=33, tiles_n=4, zero_fill=0),
         tb=True, acc=True, fallback=P("lds", 3)),
    case("kc-no-split-five-row-band", "gemm", 1600, 2048, 2048, P("kc_direct", 0, splits=1, atomic=0, map=3, tiles_m=13, tiles_n=16, grid=208),
         bias=True),
    case("kc-nt-ragged-strided", "gemm", 130, 200, 2048, P("kc_direct", 1, splits=8, map=1, grid=32), tb=True, lda=2052, ldb=2052, ldc=204,
         bias=True, acc=True, fallback=P("lds", 3, a_vec=1, b_vec=1)),
    # ---- gemm_f32_kernel<A_KC, B_KC> (LDS): variant = A_KC * 2 + B_KC; the four layouts, scalar loads per operand, split K
    case("lds-nn", "gemm", 100, 80, 40, P("lds", 2, splits=1, atomic=0, map=0, a_vec=1, b_vec=1, grid=1), bias=True, fallback=P("lds", 2)),
    case("lds-tn-odd-lda", "gemm", 257, 130, 33, P("lds", 0, a_vec=0, b_vec=0, grid=6), ta=True, fallback=P("lds", 0, a_vec=0)),
    case("lds-nt", "gemm", 16, 16, 4, P("lds", 3, a_vec=1, b_vec=1), tb=True, acc=True, fallback=P("lds", 3)),
    case("lds-tt-split-xcd", "gemm", 64, 128, 5000, P("lds", 1, splits=19, k_chunk=272, atomic=1, zero_fill=1, map=1, grid=19), ta=True, tb=True,
         fallback=P("lds", 1, splits=19)),
    case("lds-nn-odd-ldb", "gemm", 100, 80, 40, P("lds", 2, a_vec=1, b_vec=0), ldb=81, bias=True, acc=True),
    case("lds-nn-a-offset", "gemm", 100, 80, 40, P("lds", 2, a_vec=0, b_vec=1), off=(1, 0, 0)),
    case("lds-tt-b-offset-c-offset", "gemm", 100, 80, 40, P("lds", 1, a_vec=1, b_vec=0), ta=True, tb=True, off=(0, 1, 1), lda=104, ldc=83),
    case("lds-colsum", "linear_bwd", 40, 96, 777, P("lds", 0, splits=3, atomic=1, zero_fill=0), fallback=P("lds", 0, splits=3)),
    # ---- colsum4_kernel (16-byte aligned rows: eight-deep loop, four-row remainder, short last row block) / colsum_kernel
    case("colsum4-3-rows", "colsum", 0, 2048, 3, None),
    case("colsum4-128-rows", "colsum", 0, 2048, 128, None),
    case("colsum4-131-rows-strided", "colsum", 0, 260, 131, None, ldb=264),
    case("colsum4-4099-rows", "colsum", 0, 260, 4099, None, ldb=264),
    case("colsum-scalar-130-cols", "colsum", 0, 130, 131, None),
    case("colsum-scalar-odd-ld", "colsum", 0, 260, 4099, None, ldb=263),
    # ---- reduced precision through the front door, the cases of the first table (kept: same names, same plans)
    case("bf3-kernel", "gemm", 256, 200, 512, P("bf3", 2, splits=1), precision=1, bias=True),
    case("bf3-kernel-tn-acc", "gemm", 130, 128, 1024, P("bf3", 0, splits=2, atomic=1), precision=1, ta=True, acc=True),
    case("bf3-falls-back-k-tail", "gemm", 100, 80, 40, P("lds", 2), precision=1, bias=True),
    case("bf16-kernel", "gemm", 256, 200, 512, P("bf3", 7), precision=2, tb=True, bias=True),
    case("bf16-falls-back-k-tail", "gemm", 300, 64, 20, P("skinny_k", 6), precision=2),
]


def _bf3_cases(precision):
    """gemm_bf3_kernel<A_KC, B_KC, SINGLE>: variant = single * 4 + A_KC * 2 + B_KC (A_KC = !ta, B_KC = tb); tile 128 x 128, K steps of
    32, a split needs K >= 1024.  The same layouts for bf16x3 (v0 .. v3) and plain bf16 (v4 .. v7)."""
    n, v = ("bf3", 0) if precision == 1 else ("bf16", 4)
    c = lambda name, *a, **kw: case("%s-%s" % (n, name), "gemm", *a, precision=precision, **kw)
    return [
        # both operands row contiguous, nothing a multiple of 4; the K tail (one element of the second K step) comes back as zeros
        # from the end of the buffer resource
        c("tn-odd-ld-k-tail", 130, 129, 33, P("bf3", v + 0, splits=1, k_chunk=64, atomic=0, zero_fill=0, tiles_m=2, tiles_n=2, grid=4), ta=True),
        # two splits of 544; the second has fifteen K steps and a 6-element tail
        c("tn-split-k-tail-acc", 129, 129, 1030, P("bf3", v + 0, splits=2, k_chunk=544, atomic=1, zero_fill=0, grid=8), ta=True, acc=True),
        c("tt-split-zero-fill-bias", 257, 130, 1024, P("bf3", v + 1, splits=2, k_chunk=512, atomic=1, zero_fill=1, tiles_m=3, tiles_n=2, grid=12),
          ta=True, tb=True, bias=True, ldb=1028),
    ] + ([] if precision == 1 else [      # (bf16x3: "bf3-kernel" above is this case)
        c("nn-one-split", 256, 200, 512, P("bf3", v + 2, splits=1, k_chunk=512, atomic=0, zero_fill=0, grid=4), bias=True),
    ]) + [
        c("nn-split-strided-bias-acc", 130, 200, 1024, P("bf3", v + 2, splits=2, k_chunk=512, atomic=1, zero_fill=0, grid=8), lda=1028, ldc=204,
          bias=True, acc=True),
        # a single split made atomic by accumulate alone
        c("nt-strided-bias-acc", 130, 200, 64, P("bf3", v + 3, splits=1, k_chunk=64, atomic=1, zero_fill=0, grid=4), tb=True, lda=68, ldb=72,
          ldc=204, bias=True, acc=True),
    ]


CASES += _bf3_cases(1) + _bf3_cases(2) + [
    # ---- a k-contiguous operand the kernel's 16-byte buffer loads cannot address (ld % 4 != 0; K % 32 != 0 above): the f32 ladder
    case("bf3-falls-back-odd-lda", "gemm", 130, 200, 64, P("lds", 2, a_vec=0, b_vec=1), precision=1, lda=66, bias=True),
    case("bf16-falls-back-odd-ldb", "gemm", 130, 200, 64, P("lds", 3, a_vec=1, b_vec=0), precision=2, tb=True, ldb=70, acc=True),
    # ---- gemm_bf16p_kernel behind its two operand copies: variant = A_KC * 2 + B_KC (a KC operand is converted in place, the other
    #      transposed in 64 x 64 tiles); tile 256 x 256, k tiles of 32, a ring of four stages; a split needs K >= 2048
    case("bf16p-nt-two-k-tiles", "packed", 256, 256, 64, P("bf16p", 3, splits=1, k_chunk=64, tiles_m=1, tiles_n=1, grid=1, atomic=0, zero_fill=0),
         tb=True),      # (fewer k tiles than the prologue's three fills)
    case("bf16p-nn-clamped-ring-wraps", "packed", 300, 320, 192, P("bf16p", 2, splits=1, k_chunk=192, tiles_m=2, tiles_n=2, grid=4), lda=196,
         ldb=324, ldc=324, bias=True, acc=True),      # (44 live rows in the last M tile, 64 columns in the last N tile, six k tiles)
    case("bf16p-tn-four-k-tiles", "packed", 320, 256, 128, P("bf16p", 0, splits=1, k_chunk=128, tiles_m=2, tiles_n=1, grid=2), ta=True),
    case("bf16p-tt-clamped-b", "packed", 256, 300, 320, P("bf16p", 1, splits=1, k_chunk=320, tiles_m=1, tiles_n=2, grid=2), ta=True, tb=True),
    case("bf16p-nt-split-uneven-bias-acc", "packed", 320, 256, 2112, P("bf16p", 3, splits=8, k_chunk=288, tiles_m=2, tiles_n=1, grid=16, atomic=0,
                                                                       zero_fill=0), tb=True, bias=True, acc=True, ldc=260),
    case("bf16p-tn-split-overwrite", "packed", 256, 512, 2048, P("bf16p", 0, splits=8, k_chunk=256, tiles_m=1, tiles_n=2, grid=16), ta=True),
    # ---- cvt_rows_kernel / cvt_transpose_kernel / bf16_transpose_kernel: x [K, N]
    case("copy-3x8", "copy", 0, 8, 3, None),
    case("copy-257x72-strided", "copy", 0, 72, 257, None, ldb=76),
    case("copyt-one-tile", "copy_t", 0, 64, 64, None),
    case("copyt-strided", "copy_t", 0, 192, 128, None, ldb=196, ldc=136),
    case("copyt-strided-colsum", "copy_t", 0, 192, 128, None, ldb=196, ldc=136, colsum=True),
    case("copyt-strided-plain", "copy_t", 0, 192, 128, None, ldb=196, ldc=136, plain=True),
    case("transpose16-strided", "transpose16", 0, 192, 128, None, ldc=136),
]
UNPLANNED = ("colsum", "copy", "copy_t", "transpose16")      # entries without a plan: the query is about products

# What the reduced-precision entries refuse or do not take: no plan, an error (or None) from the call, nothing written.
REFUSED = [      # A or B not 16-byte aligned: AmdSpeechError "16-byte aligned" from the call and from the plan query
    case("bf3-refuses-unaligned-a", "gemm", 130, 200, 64, None, precision=1, off=(1, 0, 0)),
    case("bf16-refuses-unaligned-b", "gemm", 130, 200, 64, None, precision=2, tb=True, off=(0, 1, 0), acc=True),
]
NOT_TAKEN = [    # amdspeech_gemm_bf16_packed_scratch_bytes == 0, ops.gemm_bf16_packed returns None, the plan query refuses
    case("bf16p-not-taken-m-255", "packed", 255, 256, 64, None, tb=True),
    case("bf16p-not-taken-k-96", "packed", 256, 256, 96, None, tb=True),
    case("bf16p-not-taken-ta-m-300", "packed", 300, 256, 64, None, ta=True, tb=True),
    case("bf16p-not-taken-n-300", "packed", 256, 300, 64, None),
    case("bf16p-not-taken-odd-lda", "packed", 256, 256, 64, None, tb=True, lda=66),
]
SCRATCH_CASE = "bf16p-nt-split-uneven-bias-acc"      # run once more with the caller's scratch: a view of exactly scratch_bytes

# Every (family, variant) the dispatch can produce (include/amdspeech.h, "variant"), and the launch properties every one of which
# must appear in some case.  test_cpu_gemm_ref.py asserts both against the table.
VARIANTS = ([("skinny_n", nt) for nt in range(1, 7)] + [("skinny_k", kt * 2 + tb) for kt in (3, 5) for tb in (0, 1)] +
            [("skinny_tn", f * 8 + r) for f, r in [(0, 1), (0, 2), (0, 3), (0, 4), (1, 0), (1, 1), (1, 2), (1, 3), (1, 4)]] +
            [("tn_direct", c) for c in (1, 2, GROUP_MAX)] + [("kc_direct", tb) for tb in (0, 1)] + [("lds", v) for v in range(4)] +
            [("bf3", v) for v in range(8)] + [("bf16p", v) for v in range(4)])
PROPERTIES = {
    "skinny-k one column slice": lambda c, p: p["family"] == "skinny_k" and p["col_slices"] == 1,
    "skinny-k two column slices": lambda c, p: p["family"] == "skinny_k" and p["col_slices"] == 2,
    "map linear": lambda c, p: p["map"] == 0 and p["family"] in ("tn_direct", "lds"),
    "map per-XCD": lambda c, p: p["map"] == 1,
    "map per-XCD blocks": lambda c, p: p["map"] == 2,
    "map kc band": lambda c, p: p["map"] == 3,
    "one split": lambda c, p: p["splits"] == 1,
    "split K": lambda c, p: p["splits"] > 1,
    "atomic from accumulate alone": lambda c, p: p["atomic"] == 1 and p["splits"] == 1 and c["acc"],
    "zero fill": lambda c, p: p["zero_fill"] == 1,
    "scalar loads of A": lambda c, p: p["a_vec"] == 0,
    "scalar loads of B": lambda c, p: p["b_vec"] == 0,
    "one problem": lambda c, p: c["count"] == 1 and p["family"] == "tn_direct",
    "two problems": lambda c, p: c["count"] == 2,
    "GROUP_MAX problems": lambda c, p: c["count"] == GROUP_MAX,
    "bf16x3 on its kernel": lambda c, p: c["precision"] == 1 and p["family"] == "bf3",
    "bf16x3 falls back": lambda c, p: c["precision"] == 1 and p["family"] != "bf3",
    "bf16 on its kernel": lambda c, p: c["precision"] == 2 and p["family"] == "bf3",
    "bf16 falls back": lambda c, p: c["precision"] == 2 and p["family"] not in ("bf3", "bf16p"),
    "bf16x3 falls back on an odd ld": lambda c, p: c["precision"] == 1 and p["family"] != "bf3" and c["K"] % 32 == 0,
    "bf16 falls back on an odd ld": lambda c, p: c["precision"] == 2 and p["family"] not in ("bf3", "bf16p") and c["K"] % 32 == 0,
    "bf16x3 falls back on a K tail": lambda c, p: c["precision"] == 1 and p["family"] != "bf3" and c["K"] % 32 != 0,
    "bf16 falls back on a K tail": lambda c, p: c["precision"] == 2 and p["family"] not in ("bf3", "bf16p") and c["K"] % 32 != 0,
    "bf3 K tail, one split": lambda c, p: p["family"] == "bf3" and c["K"] % 32 != 0 and p["splits"] == 1,
    "bf3 K tail in the last split": lambda c, p: p["family"] == "bf3" and c["K"] % 32 != 0 and p["splits"] > 1,
    "bf3 zero fill": lambda c, p: p["family"] == "bf3" and p["zero_fill"] == 1,
    "bf3 split onto prior contents": lambda c, p: p["family"] == "bf3" and p["splits"] > 1 and c["acc"],
    "bf3 atomic from accumulate alone": lambda c, p: p["family"] == "bf3" and p["atomic"] == 1 and p["splits"] == 1 and c["acc"],
    "bf3 ragged rows and columns": lambda c, p: p["family"] == "bf3" and c["M"] % 128 and c["N"] % 128,
    "bf3 strided k-contiguous A": lambda c, p: p["family"] == "bf3" and not c["ta"] and c["lda"],
    "bf3 strided k-contiguous B": lambda c, p: p["family"] == "bf3" and c["tb"] and c["ldb"],
    "bf3 strided C": lambda c, p: p["family"] == "bf3" and c["ldc"],
    "packed: fewer k tiles than the prologue fills": lambda c, p: p["family"] == "bf16p" and c["K"] // 32 < 3,
    "packed: the ring wraps": lambda c, p: p["family"] == "bf16p" and p["splits"] == 1 and c["K"] // 32 > 4,
    "packed: clamped A rows": lambda c, p: p["family"] == "bf16p" and c["M"] % 256,
    "packed: clamped B rows": lambda c, p: p["family"] == "bf16p" and c["N"] % 256,
    "packed: strided operands and result": lambda c, p: p["family"] == "bf16p" and c["lda"] and c["ldb"] and c["ldc"],
    "packed: split K, short last split": lambda c, p: p["family"] == "bf16p" and p["splits"] > 1 and c["K"] % p["k_chunk"],
    "packed: split K, even": lambda c, p: p["family"] == "bf16p" and p["splits"] > 1 and c["K"] % p["k_chunk"] == 0,
    "packed: reduce with bias onto prior contents": lambda c, p: p["family"] == "bf16p" and p["splits"] > 1 and c["bias"] and c["acc"],
    "packed: reduce overwrites": lambda c, p: p["family"] == "bf16p" and p["splits"] > 1 and not c["acc"],
    "packed: one pass with bias onto prior contents": lambda c, p: p["family"] == "bf16p" and p["splits"] == 1 and c["bias"] and c["acc"],
}
COPY_PROPERTIES = {      # ... and of the cases without a plan
    "plain copy, fewer values than a workgroup": lambda c: c["entry"] == "copy" and c["K"] * c["N"] < 256 * 8,
    "plain copy, strided, a partial last workgroup": lambda c: c["entry"] == "copy" and c["ldb"] and (c["K"] * c["N"] // 8) % 256,
    "transposing copy, one tile": lambda c: c["entry"] == "copy_t" and c["K"] == c["N"] == 64,
    "transposing copy, strided on both sides": lambda c: c["entry"] == "copy_t" and c["ldb"] and c["ldc"] and not c["colsum"] and not c["plain"],
    "transposing copy with column sums": lambda c: c["entry"] == "copy_t" and c["colsum"],
    "transposing copy with the plain second output": lambda c: c["entry"] == "copy_t" and c["plain"],
    "bf16 transpose, strided": lambda c: c["entry"] == "transpose16" and c["ldc"],
}


def by_name(name):
    return next(c for c in CASES + REFUSED + NOT_TAKEN if c["name"] == name)


def shapes(c):
    """Storage shapes and row strides: {"A": (rows, cols, ld), "B": ..., "C": ...} (colsum and copy cases: B is x; copies: C is dst)."""
    a = (c["K"], c["M"]) if c["ta"] else (c["M"], c["K"])
    b = (c["N"], c["K"]) if c["tb"] else (c["K"], c["N"])
    cc = (c["M"], c["N"])
    if c["entry"] == "copy":
        cc = (c["K"], c["N"])
    if c["entry"] in ("copy_t", "transpose16"):
        cc = (c["N"], c["K"])
    return {"A": a + (c["lda"] or a[1],), "B": b + (c["ldb"] or b[1],), "C": cc + (c["ldc"] or cc[1],)}


def plan_args(c):
    """Arguments of ops.gemm_plan for a case: shapes, strides and NOMINAL addresses that carry the case's alignment."""
    sh = shapes(c)
    addr = lambda i: 4096 + 4 * c["off"][i]
    return dict(a=sh["A"] + (addr(0),), b=sh["B"] + (addr(1),), out=sh["C"] + (addr(2),), trans_a=c["ta"], trans_b=c["tb"], bias=bool(c["bias"]),
                accumulate=c["acc"], colsum=c["colsum"] and c["entry"] != "tn_group", count=c["count"], precision=c["precision"])


def query(ops, c):
    """The library's plan for a case: ops.gemm_plan, or ops.gemm_bf16_packed_plan for the packed path (None: the entry has no plan)."""
    if c["entry"] in UNPLANNED:
        return None
    if c["entry"] == "packed":
        sh = shapes(c)
        return ops.gemm_bf16_packed_plan(sh["A"], sh["B"], trans_a=c["ta"], trans_b=c["tb"])
    return ops.gemm_plan(**plan_args(c))


# ---- the recorded plan sweep: tests/golden/gemm_plans.npz, written by tools/make_golden.py --gemm-plans from the build of the commit
# BEFORE a change of the planning code; test_cpu_gemm_ref.py holds today's answers against it, field for field, in both switch modes.
SWEEP_COLUMNS = ("entry", "precision", "ta", "tb", "M", "N", "K", "lda", "ldb", "ldc", "offa", "offb", "offc", "bias", "acc", "colsum", "count")
SWEEP_GEMM, SWEEP_PACKED = 0, 1      # column "entry": ops.gemm_plan / ops.gemm_bf16_packed_plan
SWEEP_FILE = "gemm_plans.npz"


def sweep_row(c):
    """A case of the table above as a row of the sweep."""
    sh = shapes(c)
    return (SWEEP_PACKED if c["entry"] == "packed" else SWEEP_GEMM, c["precision"], int(c["ta"]), int(c["tb"]), c["M"], c["N"], c["K"],
            sh["A"][2], sh["B"][2], sh["C"][2]) + tuple(c["off"]) + (int(bool(c["bias"])), int(c["acc"]),
            int(c["colsum"] and c["entry"] != "tn_group"), c["count"])


def sweep_call(ops, row):
    """The plan query one row names (ld* in elements; off*: element offset of the nominal address, 1 = aligned to 4 bytes only)."""
    r = dict(zip(SWEEP_COLUMNS, (int(v) for v in row)))
    a = (r["K"], r["M"]) if r["ta"] else (r["M"], r["K"])
    b = (r["N"], r["K"]) if r["tb"] else (r["K"], r["N"])
    if r["entry"] == SWEEP_PACKED:
        return ops.gemm_bf16_packed_plan(a + (r["lda"],), b + (r["ldb"],), trans_a=bool(r["ta"]), trans_b=bool(r["tb"]))
    return ops.gemm_plan(a=a + (r["lda"], 4096 + 4 * r["offa"]), b=b + (r["ldb"], 4096 + 4 * r["offb"]),
                         out=(r["M"], r["N"], r["ldc"], 4096 + 4 * r["offc"]), trans_a=bool(r["ta"]), trans_b=bool(r["tb"]), bias=bool(r["bias"]),
                         accumulate=bool(r["acc"]), colsum=bool(r["colsum"]), count=r["count"], precision=r["precision"])


def sweep_answers(ops, calls, fields, messages):
    """Today's answer to every row: (plans [n, len(fields)] int32 with the family as its index in lib.GEMM_FAMILIES, status [n] int32).
    status -1: planned; >= 0: refused (the plan row stays zero), with the index of the message's CLASS -- the library's text with every
    word that is a number replaced by '#' -- in `messages`, which is extended by classes it does not hold yet."""
    from rnn_speech_amd import lib
    plans = np.zeros((len(calls), len(fields)), np.int32)
    status = np.full(len(calls), -1, np.int32)
    for i, row in enumerate(calls):
        try:
            p = sweep_call(ops, row)
        except lib.AmdSpeechError as e:
            cls = " ".join("#" if word.isdigit() else word for word in str(e).split("): ", 1)[1].split(" "))
            if cls not in messages:
                messages.append(cls)
            status[i] = messages.index(cls)
            continue
        p["family"] = lib.GEMM_FAMILIES.index(p["family"])
        plans[i] = [p[f] for f in fields]
    return plans, status


def arith(c, plan):
    """How a product carries one operand value: "f32" (all 24 bits; also where reduced precision falls back to the f32 ladder),
    "bf16x3" (hi + lo) or "bf16"."""
    if plan is None or plan["family"] not in ("bf3", "bf16p"):
        return "f32"
    return "bf16x3" if c["precision"] == 1 else "bf16"


# ---- bf16 in numpy (finite values that do not round to infinity) --------------------------------------------------------------------
def bf16_bits(x):
    """Round to nearest even: the upper 16 bits of the rounded f32, as uint16."""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def bf16_rne(x):
    return (bf16_bits(x).astype(np.uint32) << 16).view(np.float32)


def bf16_trunc(x):
    """(the planted fault: the low 16 bits cut off)"""
    return (np.ascontiguousarray(x, np.float32).view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)


def split2(x, rnd=bf16_rne):
    """hi = rnd(x), lo = rnd(x - hi), the subtraction in f32 (exact): gemm_bf3.hip, split8."""
    x = np.ascontiguousarray(x, np.float32)
    hi = rnd(x)
    return hi, rnd(x - hi)


def carried(x, how):
    """The f32 value a product returns for operand value x times an exact 1: arith()."""
    if how == "f32":
        return np.ascontiguousarray(x, np.float32)
    if how == "bf16":
        return bf16_rne(x)
    hi, lo = split2(x)
    out = hi.astype(np.float64) + lo.astype(np.float64)
    assert np.array_equal(out.astype(np.float32).astype(np.float64), out)      # (f32 holds hi + lo exactly)
    return out.astype(np.float32)


def emulate(c, o, plan, fault=None):
    """The arithmetic of the reduced-precision kernels restated for ONE problem whose terms are exact (ints, select): rounded planes,
    K ranges of the plan, steps of 32, partial results summed; f32 result.  fault: None, or a planted one --
      "a_lo" / "b_lo"       that operand's lo plane dropped (bf16x3)
      "trunc"               truncation instead of round to nearest even
      "last_k_step"         the last 32-step of every K range dropped
      "split_not_reduced"   the last K range's partial result left out"""
    how = arith(c, plan)
    assert how != "f32"
    A = (o["A"].T if c["ta"] else o["A"]).astype(np.float32)
    B = (o["B"].T if c["tb"] else o["B"]).astype(np.float32)
    rnd = bf16_trunc if fault == "trunc" else bf16_rne
    (Ah, Al), (Bh, Bl) = split2(A, rnd), split2(B, rnd)
    if how == "bf16" or fault == "a_lo":
        Al = np.zeros_like(Al)
    if how == "bf16" or fault == "b_lo":
        Bl = np.zeros_like(Bl)
    Ah, Al, Bh, Bl = (x.astype(np.float64) for x in (Ah, Al, Bh, Bl))
    K = c["K"]
    chunk = plan["k_chunk"] if plan["splits"] > 1 else K
    total = np.zeros((c["M"], c["N"]), np.float64)
    for j, k0 in enumerate(range(0, K, chunk)):
        k1 = min(K, k0 + chunk)
        if fault == "last_k_step":
            k1 = k0 + ((k1 - k0 + 31) // 32 - 1) * 32
        if fault == "split_not_reduced" and j == plan["splits"] - 1:
            continue
        k = slice(k0, k1)
        total += Ah[:, k] @ Bh[k] + Ah[:, k] @ Bl[k] + Al[:, k] @ Bh[k]
    out = total.astype(np.float32)
    assert np.array_equal(out.astype(np.float64), total)      # exact terms only
    if o["bias"] is not None:
        out = out + o["bias"]
    if o["C0"] is not None:
        out = o["C0"] + out
    return out


KINDS = ("ints", "selA", "selB", "normal")


def kinds(c):
    return ("ints", "normal") if c["entry"] in UNPLANNED else KINDS


def copy_values(rng, rows, cols):
    """f32 values for the converting copies: randn across magnitudes 2^-60 .. 2^60, and -- planted at the start of the first rows, both
    signs -- +-0, exact ties whose even neighbour lies below and above, values one f32 ulp to either side of a tie, mantissas that
    carry into the next power of two (from a tie and from all ones), the largest and smallest mantissa.  No NaN, no denormal,
    nothing that rounds to infinity."""
    x = (rng.randn(rows, cols) * np.exp2(rng.randint(-60, 61, size=(rows, cols)))).astype(np.float32)
    bits = [0x00000000, 0x3F808000, 0x3F818000, 0x3F808001, 0x3F807FFF, 0x3F818001, 0x3F817FFF, 0x3F7F8000, 0x3FFFFFFF, 0x3F7FFFFF,
            0x3F800001, 0x3F80FFFF, 0x5D7F8000, 0x217F8000, 0x5D808000, 0x21818000]
    special = np.array(bits + [b | 0x80000000 for b in bits], np.uint32).view(np.float32)
    flat = x.reshape(-1)
    n = min(len(special), flat.size)
    flat[:n] = special[:n]
    if rows > 1 and cols >= 8:      # ... and once more down a column: the transposing copies handle rows and columns differently
        m = min(len(special), rows - 1)
        x[1:1 + m, cols - 3] = special[:m]
    return x


def copy_operands(c, kind, rng):
    import torch
    rows, cols = c["K"], c["N"]
    x = rng.randint(-3, 4, size=(rows, cols)).astype(np.float32) if kind == "ints" else copy_values(rng, rows, cols)
    ref = torch.from_numpy(x).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)      # [rows, cols] bits
    o = dict(B=x, P=ref if c["plain"] else None, cs0=None)
    if c["entry"] == "transpose16":
        o["B"] = ref      # (the source IS bf16)
    o["D"] = ref if c["entry"] == "copy" else np.ascontiguousarray(ref.T)
    if c["colsum"]:
        cs0 = rng.randint(-3, 4, size=cols).astype(np.float32) if kind == "ints" else copy_values(rng, 1, cols)[0]
        o.update(cs0=cs0, cs=cs0.astype(np.float64) + x.astype(np.float64).sum(0), cs_exact=kind == "ints")
    return o


def select_indices(n, K, plan):
    """n indices into the K axis: 0, K - 1, both sides of every split boundary of the plan, the rest spread evenly."""
    edges = []
    if plan and plan.get("splits", 1) > 1:
        for j in range(1, plan["splits"]):
            b = j * plan["k_chunk"]
            edges += [k for k in (b - 1, b) if 0 < k < K - 1]
    if len(edges) > n - 2:                      # (more boundaries than indices: an even subset of them)
        edges = [edges[i * len(edges) // (n - 2)] for i in range(n - 2)]
    must = [0, K - 1] + edges
    spread = np.linspace(0, K - 1, num=n).round().astype(np.int64)
    idx = np.array((must + list(spread))[:n], np.int64)
    return np.random.RandomState(n + K).permutation(idx)


def operands(c, kind, plan=None):
    """Per problem: A, B in STORAGE layout (f32), bias, the prior contents C0 / cs0 (None where the call overwrites / has none),
    and the references `C` / `cs` -- int64-exact for ints (as float64), f32 for select (the selected elements as the plan's arithmetic
    carries them: `sel`, from `sel_raw`), float64 for normal -- with `exact` flags.  Copy cases: copy_operands()."""
    M, N, K = c["M"], c["N"], c["K"]
    seed = sum(ord(ch) * (i + 1) for i, ch in enumerate(c["name"])) + KINDS.index(kind) * 7919
    rng = np.random.RandomState(seed % (2 ** 31))
    ints = lambda *s: rng.randint(-3, 4, size=s).astype(np.float32)
    randn = lambda *s: rng.randn(*s).astype(np.float32)
    probs = []
    if c["entry"] in ("copy", "copy_t", "transpose16"):
        return [copy_operands(c, kind, rng)]
    how = arith(c, plan)
    for i in range(c["count"]):
        o = {}
        if c["entry"] == "colsum":
            x = ints(K, N) if kind == "ints" else randn(K, N)
            cs0 = ints(N) if kind == "ints" else randn(N)
            probs.append(dict(B=x, cs0=cs0, cs=cs0.astype(np.float64) + x.astype(np.float64).sum(0), cs_exact=kind == "ints"))
            continue
        draw = ints if kind == "ints" else randn
        A, B = draw(M, K), draw(K, N)          # logical [M, K], [K, N]
        if kind == "selA":
            A = np.zeros((M, K), np.float32)
            A[np.arange(M), select_indices(M, K, plan)] = 1.0
        if kind == "selB":
            B = np.zeros((K, N), np.float32)
            B[select_indices(N, K, plan), np.arange(N)] = 1.0
        bias = None
        if c["bias"]:
            bias = np.zeros(N, np.float32) if kind in ("selA", "selB") else draw(N)      # (select: the sum must stay exact)
        C0 = draw(M, N) if c["acc"] else None
        with_cs = c["colsum"] and (c["entry"] != "tn_group" or i % 2 == 0)
        cs0 = draw(N) if with_cs else None
        if kind in ("selA", "selB"):
            raw = B[np.argmax(A, 1), :] if kind == "selA" else A[:, np.argmax(B, 0)]
            sel = carried(raw, how)                                  # (exact f32: the element itself)
            ref = sel if C0 is None else C0 + sel                    # f32 + f32 -> f32: the one rounding of the accumulate
            assert ref.dtype == np.float32
            exact = True
            o.update(sel_raw=raw, sel=sel)
        else:
            ref = A.astype(np.float64) @ B.astype(np.float64)
            if bias is not None:
                ref = ref + bias
            if C0 is not None:
                ref = ref + C0
            exact = kind == "ints"
        o.update(A=np.ascontiguousarray(A.T) if c["ta"] else A, B=np.ascontiguousarray(B.T) if c["tb"] else B, bias=bias, C0=C0, cs0=cs0,
                 C=ref, exact=exact)
        if with_cs:
            # column sums of B: integers (ints) or counts of ones (selB) are exact; randn sums are judged like a product
            o.update(cs=cs0.astype(np.float64) + B.astype(np.float64).sum(0), cs_exact=kind in ("ints", "selB"))
        probs.append(o)
    return probs


def normal_bound(c, fam):
    """(absolute bound or None, relative bound or None) of the `normal` kind: tests/test_gpu_kernels.py's, per arithmetic."""
    if fam not in ("bf3", "bf16p"):
        return None, REL_TOL
    f = 8 if c["acc"] else 4
    return (6e-5 if c["precision"] == 1 else 2e-6) * np.sqrt(c["K"]) * f, None


def rel_err(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return float(np.abs(got - ref).max() / (np.abs(ref).max() + 1e-30))


def bits_equal(got, ref):
    """Bit-for-bit as f32, except that +0 and -0 compare equal (an exact zero sum has no defined sign across summation orders)."""
    got, ref = np.asarray(got, np.float32), np.asarray(ref).astype(np.float32)
    return bool(np.array_equal(got, ref))


def mismatches(got, ref, limit=6):
    got, ref = np.asarray(got, np.float32), np.asarray(ref).astype(np.float32)
    bad = np.argwhere(~(got == ref))
    head = ", ".join("%s got %r want %r" % (tuple(int(v) for v in i), float(got[tuple(i)]), float(ref[tuple(i)])) for i in bad[:limit])
    if got.ndim == 2 and len(bad):
        head += " | rows %d..%d cols %d..%d" % (bad[:, 0].min(), bad[:, 0].max(), bad[:, 1].min(), bad[:, 1].max())
    return "%d of %d elements differ: %s" % (len(bad), got.size, head)


# ---- placement ------------------------------------------------------------------------------------------------------------------
PAD16_IN = 0x7FC0         # bf16 NaN: surroundings of a bf16 input
PAD16_OUT = 0x40E0        # bf16 7.0: surroundings of a bf16 output
FILL16 = 0xC0A0           # bf16 -5.0: the prior contents of a bf16 output, which the copy must replace


class Placed:
    """One operand as a strided device view into a larger buffer: [guard row | rows x ld | guard row] (+ the element offset).
    dtype np.float32, or np.uint16 for bf16 bits (an int16 tensor; `pad` is then the bit pattern)."""

    def __init__(self, arr, ld, off, pad, fill=None, dtype=np.float32):
        import torch
        arr2 = arr if arr.ndim == 2 else arr[None, :]
        rows, cols = arr2.shape
        self.ld = ld = ld or cols
        assert ld >= cols
        self.dtype = np.dtype(dtype)
        self.bits = {4: np.uint32, 2: np.uint16}[self.dtype.itemsize]
        self.pad = self.dtype.type(pad)
        per16 = 16 // self.dtype.itemsize
        self.base = (ld + per16 - 1) // per16 * per16 + off   # (one guard row, rounded up to 16 bytes: the base is aligned unless `off` says otherwise)
        host = np.full((rows + 2) * ld + 2 * per16, self.pad, self.dtype)
        self.mask = np.zeros(host.size, bool)
        pos = self.base + (np.arange(rows)[:, None] * ld + np.arange(cols)[None, :])
        self.mask[pos] = True
        host[pos] = arr2 if fill is None else fill
        self.buf = torch.from_numpy(host if self.dtype.itemsize == 4 else host.view(np.int16)).cuda()
        v = torch.as_strided(self.buf, (rows, cols), (ld, 1), self.base)
        self.view = v if arr.ndim == 2 else v[0]
        assert self.view.data_ptr() % 16 == self.dtype.itemsize * off % 16

    def result(self):
        return self.view.cpu().numpy().view(self.dtype)

    def surroundings_intact(self):
        host = self.buf.cpu().numpy().view(self.dtype)
        return bool(np.array_equal(host[~self.mask].view(self.bits), np.full(int((~self.mask).sum()), self.pad).view(self.bits)))


def mismatches16(got, ref, limit=6):
    """... of two arrays of bf16 bits."""
    bad = np.argwhere(got != ref)
    head = ", ".join("%s got %#06x want %#06x" % (tuple(int(v) for v in i), int(got[tuple(i)]), int(ref[tuple(i)])) for i in bad[:limit])
    if len(bad):
        head += " | rows %d..%d cols %d..%d" % (bad[:, 0].min(), bad[:, 0].max(), bad[:, 1].min(), bad[:, 1].max())
    return "%d of %d elements differ: %s" % (len(bad), got.size, head)


def place(c, probs):
    """Device views of every operand of every problem: {"A", "B", "bias", "C", "cs"} -> Placed (or None).  C holds its prior contents
    (accumulate) or -5.0, which an overwriting call must replace.  Copy cases: {"B", "D" (dst), "P" (plain), "cs"}."""
    sh = shapes(c)
    out = []
    for o in probs:
        d = {}
        if c["entry"] == "colsum":
            d["B"] = Placed(o["B"], sh["B"][2], c["off"][1], PAD_IN)
            d["cs"] = Placed(o["cs0"], None, 0, PAD_OUT)
            out.append(d)
            continue
        if c["entry"] in ("copy", "copy_t", "transpose16"):
            if c["entry"] == "transpose16":
                d["B"] = Placed(o["B"], None, 0, PAD16_IN, dtype=np.uint16)
            else:
                d["B"] = Placed(o["B"], sh["B"][2], 0, PAD_IN)
            d["D"] = Placed(o["D"], sh["C"][2], 0, PAD16_OUT, fill=FILL16, dtype=np.uint16)
            d["P"] = Placed(o["P"], None, 0, PAD16_OUT, fill=FILL16, dtype=np.uint16) if o["P"] is not None else None
            d["cs"] = Placed(o["cs0"], None, 0, PAD_OUT) if o["cs0"] is not None else None
            out.append(d)
            continue
        d["A"] = Placed(o["A"], sh["A"][2], c["off"][0], PAD_IN)
        d["B"] = Placed(o["B"], sh["B"][2], c["off"][1], PAD_IN)
        d["bias"] = Placed(o["bias"], None, 0, PAD_IN) if o["bias"] is not None else None
        C0 = o["C0"] if o["C0"] is not None else np.full((c["M"], c["N"]), -5.0, np.float32)
        d["C"] = Placed(C0, sh["C"][2], c["off"][2], PAD_OUT)
        d["cs"] = Placed(o["cs0"], None, 0, PAD_OUT) if o["cs0"] is not None else None
        out.append(d)
    return out
