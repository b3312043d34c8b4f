"""CPU checks of tests/gemm_ref.py: every case's expected plan equals amdspeech_gemm_plan / amdspeech_gemm_bf16_packed_plan (the table
cannot drift from the dispatch), the table reaches every kernel variant the dispatch can produce, the exact references are right --
for reduced precision: a numpy restatement of the three arithmetics reproduces them, and every planted fault breaks the case written
for it -- and the plan queries refuse what the calls refuse.  No GPU: the queries inspect their pointers for null and alignment only."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gemm_ref as R  # noqa: E402

PLANNED = [c for c in R.CASES if c["entry"] not in R.UNPLANNED]
REDUCED = [c for c in PLANNED if c["precision"] != 0]      # (on their kernels or falling back: arith() says which)


@pytest.fixture(scope="module")
def ops():
    import __graft_entry__ as g
    g.build()
    from rnn_speech_amd import ops as o
    return o


def plan_mismatches(ops, mode):
    bad = []
    for c in PLANNED:
        if mode not in c["plan"]:
            continue
        got = R.query(ops, c)
        diff = {k: (v, got[k]) for k, v in c["plan"][mode].items() if got[k] != v}
        if diff:
            bad.append((c["name"], diff))
    return bad


def test_every_expected_plan_is_the_plan_of_the_dispatch(ops):
    assert os.environ.get("AMDSPEECH_GEMM_DIRECT", "1") != "0" and os.environ.get("AMDSPEECH_GEMM_KC_DIRECT", "1") != "0"
    assert len({c["name"] for c in R.CASES}) == len(R.CASES)
    bad = plan_mismatches(ops, "default")
    assert not bad, bad


def test_every_expected_plan_under_the_fallback_switches(ops):
    """AMDSPEECH_GEMM_DIRECT=0 AMDSPEECH_GEMM_KC_DIRECT=0 are read once per process: one child process plans every case that names a
    plan for that mode."""
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "import test_cpu_gemm_ref as T\nfrom rnn_speech_amd import ops\n"
            "bad = T.plan_mismatches(ops, 'fallback')\nprint('FALLBACK-PLANS', sum('fallback' in c['plan'] for c in T.PLANNED), bad)\n"
            "sys.exit(1 if bad else 0)\n" % (ROOT, os.path.join(ROOT, "tests")))
    out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **R.FALLBACK_ENV), capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    n = sum("fallback" in c["plan"] for c in PLANNED)
    assert n >= 8 and "FALLBACK-PLANS %d []" % n in out.stdout, out.stdout[-2000:]
    # ... and there every one of them is on the LDS kernel
    assert all(c["plan"]["fallback"]["family"] == "lds" for c in PLANNED if "fallback" in c["plan"])


def sweep_mismatches(ops, mode):
    """Rows of tests/golden/gemm_plans.npz whose recorded answer (plan fields, or refusal and message class) is not today's."""
    from rnn_speech_amd import lib
    g = np.load(os.path.join(ROOT, "tests", "golden", R.SWEEP_FILE))
    fields, messages = [str(f) for f in g["fields"]], [str(m) for m in g["messages"]]
    assert tuple(str(c) for c in g["columns"]) == R.SWEEP_COLUMNS and fields == [n for n, _ in lib.GemmPlanInfo._fields_]
    assert tuple(str(f) for f in g["families"]) == lib.GEMM_FAMILIES
    plans, status = R.sweep_answers(ops, g["calls"], fields, messages)
    want_plans, want_status = g["plans_" + mode], g["status_" + mode]
    bad = np.flatnonzero((plans != want_plans).any(1) | (status != want_status))
    text = lambda s: "planned" if s < 0 else "refused: " + messages[s]
    return [(dict(zip(R.SWEEP_COLUMNS, g["calls"][i].tolist())), text(want_status[i]), text(status[i]),
             {f: (int(w), int(p)) for f, w, p in zip(fields, want_plans[i], plans[i]) if w != p}) for i in bad[:20]], len(status)


def test_every_recorded_plan_of_the_sweep_is_todays_plan(ops):
    """The file was written by the build of the commit before the planning code was last restructured (tools/make_golden.py
    --gemm-plans): 79 thousand calls over shapes, layouts, options, strides and alignments."""
    from rnn_speech_amd import lib
    assert os.environ.get("AMDSPEECH_GEMM_DIRECT", "1") != "0" and os.environ.get("AMDSPEECH_GEMM_KC_DIRECT", "1") != "0"
    g = np.load(os.path.join(ROOT, "tests", "golden", R.SWEEP_FILE))
    planned = g["plans_default"][g["status_default"] < 0]
    seen = {(lib.GEMM_FAMILIES[f], int(v)) for f, v in np.unique(planned[:, :2], axis=0)}
    assert {f for f, _ in seen} == set(lib.GEMM_FAMILIES) and set(R.VARIANTS) <= seen
    assert (g["status_default"] >= 0).sum() > 1000 and len({str(m) for m in g["messages"]}) >= 3      # refusals are recorded as such
    fallback = {lib.GEMM_FAMILIES[f] for f in np.unique(g["plans_fallback"][g["status_fallback"] < 0][:, 0])}
    assert "lds" in fallback and not fallback & {"tn_direct", "kc_direct"}      # (the second mode was recorded with the switches off)
    bad, n = sweep_mismatches(ops, "default")
    assert n == len(g["calls"]) > 50000 and not bad, bad


def test_every_recorded_plan_of_the_sweep_under_the_fallback_switches(ops):
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "import test_cpu_gemm_ref as T\nfrom rnn_speech_amd import ops\n"
            "bad, n = T.sweep_mismatches(ops, 'fallback')\nprint('FALLBACK-SWEEP', n, bad)\n"
            "sys.exit(1 if bad else 0)\n" % (ROOT, os.path.join(ROOT, "tests")))
    out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **R.FALLBACK_ENV), capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    n = len(np.load(os.path.join(ROOT, "tests", "golden", R.SWEEP_FILE))["calls"])
    assert "FALLBACK-SWEEP %d []" % n in out.stdout, out.stdout[-2000:]


def test_the_table_reaches_every_variant_and_every_launch_property(ops):
    from rnn_speech_amd import lib
    assert R.GROUP_MAX == lib.GEMM_GROUP_MAX
    header = open(os.path.join(ROOT, "include", "amdspeech.h")).read()
    assert "AMDSPEECH_GEMM_GROUP_MAX = %d" % R.GROUP_MAX in header
    plans = [(c, R.query(ops, c)) for c in PLANNED]
    seen = {(p["family"], p["variant"]) for _, p in plans}
    missing = [v for v in R.VARIANTS if v not in seen]
    assert not missing, missing
    assert {f for f, _ in R.VARIANTS} == set(lib.GEMM_FAMILIES)      # no family without an enumeration
    assert "AMDSPEECH_GEMM_BF16P = %d" % lib.GEMM_FAMILIES.index("bf16p") in header
    uncovered = [name for name, holds in R.PROPERTIES.items() if not any(holds(c, p) for c, p in plans)]
    assert not uncovered, uncovered
    uncovered = [name for name, holds in R.COPY_PROPERTIES.items() if not any(holds(c) for c in R.CASES)]
    assert not uncovered, uncovered
    # every case names family and variant, every case of the table is planned or is a column-sum case: nothing is left out
    assert all({"family", "variant"} <= set(c["plan"]["default"]) for c in PLANNED)
    assert len(PLANNED) + sum(c["entry"] in ("colsum", "copy", "copy_t", "transpose16") for c in R.CASES) == len(R.CASES)
    assert all(c["plan"]["default"] is None for c in R.CASES if c["entry"] in R.UNPLANNED)
    # the exactness condition of the `ints` kind: |sum| <= 9 K (+ bias and prior contents <= 6, + column sums 3 K) stays below 2^24
    assert all(9 * c["K"] + 16 < 2 ** 24 for c in R.CASES)


@pytest.mark.parametrize("name", ["tn-split-odd-k", "lds-tt-split-xcd", "skk-kt5-nt", "tng-2-blocks-ragged", "kc-one-tile-8-splits",
                                  "bf3-tn-split-k-tail-acc", "bf16p-nn-clamped-ring-wraps"])
def test_ints_reference_is_the_int64_product_in_any_f32_summation_order(ops, name):
    c = R.by_name(name)
    plan = R.query(ops, c)
    for o in R.operands(c, "ints", plan):
        A = o["A"].T if c["ta"] else o["A"]
        B = o["B"].T if c["tb"] else o["B"]
        want = A.astype(np.int64) @ B.astype(np.int64)
        if o["bias"] is not None:
            want = want + o["bias"].astype(np.int64)
        if o["C0"] is not None:
            want = want + o["C0"].astype(np.int64)
        assert o["exact"] and np.array_equal(o["C"], want.astype(np.float64))
        assert np.abs(want).max() < 2 ** 24
        start = np.zeros_like(want, dtype=np.float32)
        if o["bias"] is not None:
            start = start + o["bias"]
        if o["C0"] is not None:
            start = start + o["C0"]
        K = c["K"]
        terms = lambda k: np.outer(A[:, k], B[k, :]).astype(np.float32)
        seq = start.copy()
        for k in range(K):                       # sequential k
            seq += terms(k)
        rev = start.copy()
        for k in range(K - 1, -1, -1):           # reversed
            rev += terms(k)
        chunk = plan["k_chunk"] if plan["splits"] > 1 else (K + 2) // 3
        parts = []
        for k0 in range(0, K, chunk):            # per split, then summed (last split first, as atomics may land)
            part = np.zeros_like(start)
            for k in range(k0, min(K, k0 + chunk)):
                part += terms(k)
            parts.append(part)
        split = start.copy()
        for part in reversed(parts):
            split += part
        for got in (seq, rev, split):
            assert got.dtype == np.float32 and R.bits_equal(got, want)
        if "cs" in o:
            assert np.array_equal(o["cs"], (o["cs0"].astype(np.int64) + B.astype(np.int64).sum(0)).astype(np.float64))


@pytest.mark.parametrize("name", ["tn-split-odd-k", "lds-tt-split-xcd", "skn-nt4-ldc", "sktn-13-small-b-ldc"])
@pytest.mark.parametrize("kind", ["selA", "selB"])
def test_select_reference_is_a_float32_matmul_and_covers_the_split_boundaries(ops, name, kind):
    c = R.by_name(name)
    plan = ops.gemm_plan(**R.plan_args(c))
    (o,) = R.operands(c, kind, plan)
    A = o["A"].T if c["ta"] else o["A"]
    B = o["B"].T if c["tb"] else o["B"]
    sel = A if kind == "selA" else B
    assert set(np.unique(sel)) == {0.0, 1.0} and (sel.sum(1 if kind == "selA" else 0) == 1).all()
    prod = (A @ B).astype(np.float32)            # float32 matmul: every other term is an exact zero
    want = prod if o["C0"] is None else o["C0"] + prod
    assert o["exact"] and o["C"].dtype == np.float32 and np.array_equal(o["C"], want)
    picked = set(np.argmax(A, 1) if kind == "selA" else np.argmax(B, 0))
    must = {0, c["K"] - 1}
    if plan["splits"] > 1 and plan["family"] != "skinny_tn":
        for j in range(1, plan["splits"]):
            must |= {j * plan["k_chunk"] - 1, j * plan["k_chunk"]}
    assert must <= picked, sorted(must - picked)
    other = B if kind == "selA" else A           # full mantissas: plain bf16 (8 bits) or a bf16 pair (16 bits) cannot carry them
    assert (np.abs(other).view(np.uint32) & 0xFF).astype(bool).mean() > 0.9


def test_plan_query_refuses_what_the_call_refuses(ops):
    from rnn_speech_amd import lib
    h = lib.load()
    info = lib.GemmPlanInfo()
    P = ctypes.c_void_p
    ok = lambda **kw: h.amdspeech_gemm_plan(kw.get("precision", 0), 0, 0, kw.get("M", 100), 80, 40, P(4096), 40, P(4096), 80, P(kw.get("C", 4096)), 80,
                                            None, 0, 0, kw.get("count", 1), ctypes.byref(info))
    assert ok() == 0 and lib.GEMM_FAMILIES[info.family] == "lds"
    # a null output matrix / a non-positive shape: the message of amdspeech_gemm_f32 itself (no device is needed to refuse either)
    assert ok(C=0) != 0
    plan_msg = h.amdspeech_last_error()
    assert h.amdspeech_gemm_f32(None, 0, 0, 100, 80, 40, P(4096), 40, P(4096), 80, None, 80, None, 0) != 0
    assert h.amdspeech_last_error() == plan_msg == b"gemm: null operand"
    assert ok(M=0) != 0
    plan_msg = h.amdspeech_last_error()
    assert h.amdspeech_gemm_f32(None, 0, 0, 0, 80, 40, P(4096), 40, P(4096), 80, P(4096), 80, None, 0) != 0
    assert h.amdspeech_last_error() == plan_msg == b"gemm: non-positive shape 0 80 40"
    # the reduced-precision front door and the grouped entry likewise
    assert ok(precision=1, C=0) != 0
    plan_msg = h.amdspeech_last_error()
    assert h.amdspeech_gemm_bf16x3(None, 0, 0, 100, 80, 40, P(4096), 40, P(4096), 80, None, 80, None, 0) != 0
    assert h.amdspeech_last_error() == plan_msg == b"gemm_bf3: bad arguments"
    ptrs = (P * 2)(4096, 4096)
    assert h.amdspeech_gemm_f32_tn_group(None, 2, 0, 128, 64, ptrs, 128, ptrs, 128, ptrs, 128, None, 0) != 0
    call_msg = h.amdspeech_last_error()
    assert h.amdspeech_gemm_plan(0, 1, 0, 0, 128, 64, P(4096), 128, P(4096), 128, P(4096), 128, None, 0, 0, 2, ctypes.byref(info)) != 0
    assert h.amdspeech_last_error() == call_msg == b"gemm group: bad shape"
    # rows that are not 16-byte aligned: the grouped entry has no other kernel to fall back to
    assert h.amdspeech_gemm_f32_tn_group(None, 2, 130, 128, 64, ptrs, 130, ptrs, 128, ptrs, 128, None, 0) != 0
    call_msg = h.amdspeech_last_error()
    assert h.amdspeech_gemm_plan(0, 1, 0, 130, 128, 64, P(4096), 130, P(4096), 128, P(4096), 128, None, 0, 0, 2, ctypes.byref(info)) != 0
    assert h.amdspeech_last_error() == call_msg == b"gemm group: operand 0 does not qualify"
    assert ok(count=R.GROUP_MAX + 1) != 0 and ok(count=0) != 0 and ok(precision=3) != 0
    assert h.amdspeech_gemm_plan(0, 0, 0, 100, 80, 40, P(4096), 40, P(4096), 80, P(4096), 80, None, 0, 0, 1, None) != 0
    with pytest.raises(lib.AmdSpeechError, match="non-positive shape"):
        ops.gemm_plan((0, 40), (40, 80))


# ---- reduced precision: bf16x3, plain bf16, the packed path and its copies ---------------------------------------------------------
def test_numpy_bf16_is_torch_bf16():
    import torch
    x = np.concatenate([R.copy_values(np.random.RandomState(5), 64, 64).reshape(-1), np.random.RandomState(6).randn(100000).astype(np.float32)])
    want = torch.from_numpy(x).to(torch.bfloat16)
    assert np.array_equal(R.bf16_bits(x), want.view(torch.int16).numpy().view(np.uint16))
    assert np.array_equal(R.bf16_rne(x), want.to(torch.float32).numpy())
    assert (R.bf16_trunc(x) != R.bf16_rne(x)).mean() > 0.4


@pytest.mark.parametrize("name", [c["name"] for c in REDUCED])
def test_select_reference_of_reduced_precision_is_the_element_as_the_arithmetic_carries_it(ops, name):
    """bf16x3: hi + lo is a fixed point of the kernel's split (so the kernel owes exactly these bits) and differs from the element in more
    than 90 % of them (so the probe still proves that the arithmetic is reduced); plain bf16 and packed: the rounded element; a
    fallback: the element.  The restated arithmetic gives the same bits, and the selection covers both sides of every K range."""
    c = R.by_name(name)
    plan = R.query(ops, c)
    how = R.arith(c, plan)
    assert how == ("f32" if plan["family"] not in ("bf3", "bf16p") else "bf16x3" if c["precision"] == 1 else "bf16")
    f64 = lambda x: x.astype(np.float64)
    for kind in ("selA", "selB"):
        (o,) = R.operands(c, kind, plan)
        r, raw = o["sel"], o["sel_raw"]
        assert r.dtype == np.float32 and raw.dtype == np.float32
        if how == "f32":
            assert np.array_equal(r, raw)
            continue
        hi = R.bf16_rne(r)
        lo = R.bf16_rne((f64(r) - f64(hi)).astype(np.float32))
        assert np.array_equal((f64(r) - f64(hi)).astype(np.float32).astype(np.float64), f64(r) - f64(hi))
        if how == "bf16x3":
            assert np.array_equal(f64(hi) + f64(lo), f64(r))
            assert (np.abs(f64(r) - f64(raw)) <= np.abs(f64(raw)) * 2.0 ** -16).all()
        else:
            assert np.array_equal(hi, r) and not lo.any()
            assert (np.abs(f64(r) - f64(raw)) <= np.abs(f64(raw)) * 2.0 ** -8).all()
        assert (r != raw).mean() > 0.9
        want = r if o["C0"] is None else o["C0"] + r
        assert o["exact"] and np.array_equal(o["C"], want)
        assert R.bits_equal(R.emulate(c, o, plan), o["C"])
        picked = set(np.argmax(o["A"].T if c["ta"] else o["A"], 1) if kind == "selA" else np.argmax(o["B"].T if c["tb"] else o["B"], 0))
        must = {0, c["K"] - 1}
        for j in range(1, plan["splits"]):
            must |= {j * plan["k_chunk"] - 1, j * plan["k_chunk"]}
        assert must <= picked, sorted(must - picked)
    (o,) = R.operands(c, "ints", plan)
    if how != "f32":
        assert R.bits_equal(R.emulate(c, o, plan), o["C"])


def test_the_two_term_split_is_a_fixed_point_on_two_million_values():
    x = np.random.RandomState(3).randn(2_000_000).astype(np.float32)
    hi, lo = R.split2(x)
    r = R.carried(x, "bf16x3")
    assert np.array_equal(r.astype(np.float64), hi.astype(np.float64) + lo.astype(np.float64))
    h2, l2 = R.split2(r)      # (the PAIR may differ -- a sum that lands on a tie re-splits as (hi + ulp, -ulp / 2) -- its sum does not)
    assert np.array_equal(h2.astype(np.float64) + l2.astype(np.float64), r.astype(np.float64))
    assert 0 < (h2 != hi).mean() < 1e-2
    assert (r != x).mean() > 0.9


FAULTS = [      # (planted fault, the case written for it, the kind that must see it)
    ("a_lo", "bf3-nn-split-strided-bias-acc", "selB"),      # B selects: A's lo half travels through lo.hi and A's lo plane
    ("a_lo", "bf3-tn-odd-ld-k-tail", "selB"),
    ("b_lo", "bf3-nn-split-strided-bias-acc", "selA"),      # A selects: B's lo half travels through hi.lo and B's lo plane
    ("b_lo", "bf3-tt-split-zero-fill-bias", "selA"),
    ("trunc", "bf3-nt-strided-bias-acc", "selA"),
    ("trunc", "bf16-nt-strided-bias-acc", "selB"),
    ("trunc", "bf16p-nn-clamped-ring-wraps", "selA"),
    ("trunc", "bf16p-tn-four-k-tiles", "selB"),
    ("last_k_step", "bf3-tn-split-k-tail-acc", "ints"),     # (the 6-element tail of the second split)
    ("last_k_step", "bf3-tn-odd-ld-k-tail", "ints"),
    ("last_k_step", "bf16-tn-split-k-tail-acc", "selA"),
    ("last_k_step", "bf16p-nt-two-k-tiles", "ints"),
    ("last_k_step", "bf16p-nt-split-uneven-bias-acc", "selB"),
    ("split_not_reduced", "bf16p-nt-split-uneven-bias-acc", "ints"),
    ("split_not_reduced", "bf16p-tn-split-overwrite", "ints"),
    ("split_not_reduced", "bf16p-tn-split-overwrite", "selA"),
    ("split_not_reduced", "bf3-tt-split-zero-fill-bias", "ints"),
]


@pytest.mark.parametrize("fault,name,kind", FAULTS)
def test_a_planted_fault_breaks_the_exact_check_of_its_case(ops, fault, name, kind):
    c = R.by_name(name)
    plan = R.query(ops, c)
    (o,) = R.operands(c, kind, plan)
    assert R.bits_equal(R.emulate(c, o, plan), o["C"])
    bad = R.emulate(c, o, plan, fault=fault)
    assert not R.bits_equal(bad, o["C"])
    if fault in ("a_lo", "b_lo"):      # ... and only the probe written for that plane sees it: the other one passes
        (other,) = R.operands(c, "selA" if kind == "selB" else "selB", plan)
        assert R.bits_equal(R.emulate(c, other, plan, fault=fault), other["C"])


def test_copy_values_and_references():
    """The values of the `normal` copy kind hold what the docstring of gemm_ref promises, and the references are torch's bf16."""
    x = R.copy_values(np.random.RandomState(1), 128, 192)
    u = x.view(np.uint32)
    expo = (u >> 23) & 0xFF
    assert np.isfinite(x).all() and ((expo > 0) | (x == 0)).all() and (expo < 0xFE).all()      # no NaN / inf / denormal / near-overflow
    assert (u == 0).any() and (u == 0x80000000).any()
    low = u & 0xFFFF
    tie = low == 0x8000
    assert (tie & ((u >> 16) & 1 == 0)).sum() >= 4 and (tie & ((u >> 16) & 1 == 1)).sum() >= 4      # even below / even above
    b = R.bf16_bits(x).astype(np.uint32)
    assert ((b >> 7) != ((u >> 16) >> 7)).sum() >= 4                                            # carries into the exponent
    assert np.log2(np.abs(x[x != 0])).min() < -50 and np.log2(np.abs(x[x != 0])).max() > 50
    assert (R.bf16_bits(R.bf16_trunc(x)) != R.bf16_bits(x)).mean() > 0.4                         # (planted truncation is seen)
    for c in R.CASES:
        if c["entry"] not in ("copy", "copy_t", "transpose16"):
            continue
        for kind in R.kinds(c):
            (o,) = R.operands(c, kind)
            src = o["B"] if c["entry"] != "transpose16" else (o["B"].astype(np.uint32) << 16).view(np.float32)
            want = R.bf16_bits(src)
            assert np.array_equal(o["D"], want if c["entry"] == "copy" else want.T)
            assert (o["P"] is None) == (not c["plain"]) and (o["P"] is None or np.array_equal(o["P"], want))
            if c["colsum"]:
                assert np.array_equal(o["cs"], o["cs0"].astype(np.float64) + o["B"].astype(np.float64).sum(0))
                assert o["cs_exact"] == (kind == "ints")


def test_packed_plan_query_refuses_exactly_what_scratch_bytes_reports_as_zero(ops):
    from rnn_speech_amd import lib
    h = lib.load()
    info = lib.GemmPlanInfo()
    EINVAL = -1      # AMDSPEECH_EINVAL (include/amdspeech.h)
    n = 0
    for ta in (0, 1):
        for tb in (0, 1):
            for M in (64, 255, 256, 300, 320):
                for N in (255, 256, 300, 320):
                    for K in (32, 64, 96, 128, 2048):
                        for pad in (0, 2, 4):
                            lda, ldb = (M if ta else K) + pad, (K if tb else N) + (4 if pad else 0)
                            nbytes = h.amdspeech_gemm_bf16_packed_scratch_bytes(ta, tb, M, N, K, lda, ldb)
                            rc = h.amdspeech_gemm_bf16_packed_plan(ta, tb, M, N, K, lda, ldb, ctypes.byref(info))
                            assert (nbytes == 0) == (rc != 0), (ta, tb, M, N, K, lda, ldb, nbytes, rc)
                            if rc:
                                assert rc == EINVAL and h.amdspeech_last_error() == b"gemm_bf16_packed: shape not taken"
                            else:
                                assert lib.GEMM_FAMILIES[info.family] == "bf16p" and info.variant == (0 if ta else 2) + tb
                                assert info.atomic == 0 and info.zero_fill == 0 and info.grid == info.tiles_m * info.tiles_n * info.splits
                                assert info.k_chunk % 32 == 0 and (info.splits - 1) * info.k_chunk < K <= info.splits * info.k_chunk
                                partial = info.splits * info.tiles_m * info.tiles_n * 256 * 256 * 4 if info.splits > 1 else 0
                                up = lambda v: (v + 255) // 256 * 256
                                assert nbytes == up(M * K * 2) + up(N * K * 2) + up(partial) + 256
                            n += rc != 0
    assert n > 100
    for c in R.NOT_TAKEN:
        sh = R.shapes(c)
        assert h.amdspeech_gemm_bf16_packed_scratch_bytes(int(c["ta"]), int(c["tb"]), c["M"], c["N"], c["K"], sh["A"][2], sh["B"][2]) == 0
        with pytest.raises(lib.AmdSpeechError, match="shape not taken"):
            R.query(ops, c)
    assert h.amdspeech_gemm_bf16_packed_plan(0, 1, 256, 256, 64, 64, 64, None) != 0


def test_reduced_precision_plan_query_refuses_unaligned_operands(ops):
    from rnn_speech_amd import lib
    assert {c["precision"] for c in R.REFUSED} == {1, 2} and {c["off"] for c in R.REFUSED} == {(1, 0, 0), (0, 1, 0)}
    for c in R.REFUSED:
        with pytest.raises(lib.AmdSpeechError, match="16-byte aligned"):
            R.query(ops, c)
