"""The exact-f32 GEMM per kernel variant: the case table, exact references and operand placement of tests/test_cpu_gemm_ref.py and
tests/test_gpu_gemm_paths.py.  A checker only: the product never imports it.

Every case names ONE call (entry, precision, layouts, shape, strides, element offsets, bias / accumulate / column sums / count) and
the plan it was written for: the fields of ops.gemm_plan that matter for it.  test_cpu_gemm_ref.py holds every expected plan against
amdspeech_gemm_plan and asserts that the table reaches every (family, variant) pair the dispatch can produce (VARIANTS below).

Three operand kinds (operands()):
  ints    every operand, the bias and the prior contents of C / colsum are integers in [-3, 3] stored as f32.  Products and their sums
          are exact in f32 in ANY order while they stay below 2^24 (9 K + 16 here), split K with f32 atomics included: the result
          must equal the integer product BIT FOR BIT.  One dropped, doubled or misplaced term fails.
  select  one operand is 0/1 with exactly one 1 per output row ("selA": A selects, C[m, :] = B[k(m), :]) or per output column
          ("selB": C[:, n] = A[:, k(n)]); the other is randn with full mantissas.  k() covers 0, K - 1 and both sides of every split
          boundary.  Exact-f32 arithmetic returns all 24 bits of the selected element; split-precision arithmetic cannot.
  normal  randn operands against the float64 product of the f32 operands, rel_err < 2e-5 of max|ref|: the criterion of
          tests/test_gpu_kernels.py, not a new number.  (Reduced precision: that file's bounds for those kernels.)

place() puts every operand into a larger buffer as a strided view: one guard row before and after, ld - width padding columns.  The
INPUTS' surroundings are NaN -- a kernel that multiplies out-of-extent bytes by a zero weight fails here and passes with the zero
padding of an ordinary test; the surroundings of C and colsum are 7.0 and must still be 7.0, bit for bit, afterwards."""
import numpy as np

GROUP_MAX = 10            # AMDSPEECH_GEMM_GROUP_MAX (include/amdspeech.h)
FALLBACK_ENV = {"AMDSPEECH_GEMM_DIRECT": "0", "AMDSPEECH_GEMM_KC_DIRECT": "0"}      # everything through the LDS kernel (read once per process)
MODES = ("default", "fallback")
REL_TOL = 2e-5            # tests/test_gpu_kernels.py: rel_err of the exact-f32 GEMM
PAD_IN = float("nan")     # surroundings of the inputs
PAD_OUT = 7.0             # surroundings of the outputs


def case(name, entry, M, N, K, plan, ta=False, tb=False, lda=None, ldb=None, ldc=None, off=(0, 0, 0), bias=False, acc=False,
         colsum=False, count=1, precision=0, fallback=None):
    """M, N, K: the PRODUCT's shape (C [M, N], K the contracted axis) whatever the entry:
         gemm        ops.gemm / gemm_bf16x3 / gemm_bf16 (by precision)
         linear_bwd  ops.linear_bwd(x [K, M], w, dy [K, N], dw [M, N], db [N], need_dx=False): trans_a, accumulate, column sums of dy
         tn_group    ops.gemm_tn_group: `count` products A_i^T . B_i; colsum=True gives column sums to the EVEN problems only
         colsum      ops.colsum_accumulate(x [K, N], out [N]): no plan (the query is about products)
       ld*: None = contiguous; off: element offset of (A, B, C) into their buffers (1 = rows not 16-byte aligned)."""
    if entry == "linear_bwd":
        ta, tb, acc, colsum = True, False, True, True
    if entry == "tn_group":
        ta, tb = True, False
    plans = {"default": plan}
    if fallback is not None:
        plans["fallback"] = fallback
    return dict(name=name, entry=entry, M=M, N=N, K=K, ta=ta, tb=tb, lda=lda, ldb=ldb, ldc=ldc, off=off, bias=bias, acc=acc, colsum=colsum,
                count=count, precision=precision, plan=plans)


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
    # ---- reduced precision, front door only: the split-precision kernel, or the f32 ladder where its addressing does not fit
    case("bf3-kernel", "gemm", 256, 200, 512, P("bf3", 2, splits=1), precision=1, bias=True),
    case("bf3-kernel-tn-acc", "gemm", 130, 128, 1024, P("bf3", 0, splits=2, atomic=1), precision=1, ta=True, acc=True),
    case("bf3-falls-back-k-tail", "gemm", 100, 80, 40, P("lds", 2), precision=1, bias=True),
    case("bf16-kernel", "gemm", 256, 200, 512, P("bf3", 7), precision=2, tb=True, bias=True),
    case("bf16-falls-back-k-tail", "gemm", 300, 64, 20, P("skinny_k", 6), precision=2),
]

# Every (family, variant) the dispatch can produce (include/amdspeech.h, "variant"), and the launch properties every one of which
# must appear in some case.  test_cpu_gemm_ref.py asserts both against the table.
VARIANTS = ([("skinny_n", nt) for nt in range(1, 7)] + [("skinny_k", kt * 2 + tb) for kt in (3, 5) for tb in (0, 1)] +
            [("skinny_tn", f * 8 + r) for f, r in [(0, 1), (0, 2), (0, 3), (0, 4), (1, 0), (1, 1), (1, 2), (1, 3), (1, 4)]] +
            [("tn_direct", c) for c in (1, 2, GROUP_MAX)] + [("kc_direct", tb) for tb in (0, 1)] + [("lds", v) for v in range(4)])
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
    "bf16 falls back": lambda c, p: c["precision"] == 2 and p["family"] != "bf3",
}


def by_name(name):
    return next(c for c in CASES if c["name"] == name)


def shapes(c):
    """Storage shapes and row strides: {"A": (rows, cols, ld), "B": ..., "C": ...} (colsum cases: B is x)."""
    a = (c["K"], c["M"]) if c["ta"] else (c["M"], c["K"])
    b = (c["N"], c["K"]) if c["tb"] else (c["K"], c["N"])
    cc = (c["M"], c["N"])
    return {"A": a + (c["lda"] or a[1],), "B": b + (c["ldb"] or b[1],), "C": cc + (c["ldc"] or cc[1],)}


def plan_args(c):
    """Arguments of ops.gemm_plan for a case: shapes, strides and NOMINAL addresses that carry the case's alignment."""
    sh = shapes(c)
    addr = lambda i: 4096 + 4 * c["off"][i]
    return dict(a=sh["A"] + (addr(0),), b=sh["B"] + (addr(1),), out=sh["C"] + (addr(2),), trans_a=c["ta"], trans_b=c["tb"], bias=bool(c["bias"]),
                accumulate=c["acc"], colsum=c["colsum"] and c["entry"] != "tn_group", count=c["count"], precision=c["precision"])


KINDS = ("ints", "selA", "selB", "normal")


def kinds(c):
    return ("ints", "normal") if c["entry"] == "colsum" else KINDS


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
    and the references `C` / `cs` -- int64-exact for ints (as float64), f32 for select, float64 for normal -- with `exact` flags."""
    M, N, K = c["M"], c["N"], c["K"]
    seed = sum(ord(ch) * (i + 1) for i, ch in enumerate(c["name"])) + KINDS.index(kind) * 7919
    rng = np.random.RandomState(seed % (2 ** 31))
    ints = lambda *s: rng.randint(-3, 4, size=s).astype(np.float32)
    randn = lambda *s: rng.randn(*s).astype(np.float32)
    probs = []
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
            sel = B[np.argmax(A, 1), :] if kind == "selA" else A[:, np.argmax(B, 0)]
            ref = sel if C0 is None else C0 + sel                    # f32 + f32 -> f32: the one rounding of the accumulate
            assert ref.dtype == np.float32
            exact = True
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
    if fam != "bf3":
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
class Placed:
    """One operand as a strided device view into a larger buffer: [guard row | rows x ld | guard row] (+ the element offset)."""

    def __init__(self, arr, ld, off, pad, fill=None):
        import torch
        arr2 = arr if arr.ndim == 2 else arr[None, :]
        rows, cols = arr2.shape
        self.ld = ld = ld or cols
        assert ld >= cols
        self.pad = np.float32(pad)
        self.base = (ld + 3) // 4 * 4 + off   # (one guard row, rounded up to 16 bytes: the base is aligned unless `off` says otherwise)
        host = np.full((rows + 2) * ld + 8, self.pad, np.float32)
        self.mask = np.zeros(host.size, bool)
        pos = self.base + (np.arange(rows)[:, None] * ld + np.arange(cols)[None, :])
        self.mask[pos] = True
        host[pos] = arr2 if fill is None else fill
        self.buf = torch.from_numpy(host).cuda()
        v = torch.as_strided(self.buf, (rows, cols), (ld, 1), self.base)
        self.view = v if arr.ndim == 2 else v[0]
        assert self.view.data_ptr() % 16 == 4 * off % 16

    def result(self):
        return self.view.cpu().numpy()

    def surroundings_intact(self):
        host = self.buf.cpu().numpy()
        return bool(np.array_equal(host[~self.mask].view(np.uint32), np.full(int((~self.mask).sum()), self.pad).view(np.uint32)))


def place(c, probs):
    """Device views of every operand of every problem: {"A", "B", "bias", "C", "cs"} -> Placed (or None).  C holds its prior contents
    (accumulate) or -5.0, which an overwriting call must replace."""
    sh = shapes(c)
    out = []
    for o in probs:
        d = {}
        if c["entry"] == "colsum":
            d["B"] = Placed(o["B"], sh["B"][2], c["off"][1], PAD_IN)
            d["cs"] = Placed(o["cs0"], None, 0, PAD_OUT)
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
