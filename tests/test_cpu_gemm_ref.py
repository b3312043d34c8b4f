"""CPU checks of tests/gemm_ref.py: every case's expected plan equals amdspeech_gemm_plan (the table cannot drift from the dispatch),
the table reaches every kernel variant the dispatch can produce, the exact references are right, and the plan query refuses what the
call refuses.  No GPU: the query inspects its pointers for null and alignment only."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gemm_ref as R  # noqa: E402

PLANNED = [c for c in R.CASES if c["entry"] != "colsum"]


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
        got = ops.gemm_plan(**R.plan_args(c))
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


def test_the_table_reaches_every_variant_and_every_launch_property(ops):
    from rnn_speech_amd import lib
    assert R.GROUP_MAX == lib.GEMM_GROUP_MAX
    header = open(os.path.join(ROOT, "include", "amdspeech.h")).read()
    assert "AMDSPEECH_GEMM_GROUP_MAX = %d" % R.GROUP_MAX in header
    plans = [(c, ops.gemm_plan(**R.plan_args(c))) for c in PLANNED]
    seen = {(p["family"], p["variant"]) for _, p in plans}
    missing = [v for v in R.VARIANTS if v not in seen]
    assert not missing, missing
    assert {f for f, _ in R.VARIANTS} | {"bf3"} == set(lib.GEMM_FAMILIES)      # no family without an enumeration
    uncovered = [name for name, holds in R.PROPERTIES.items() if not any(holds(c, p) for c, p in plans)]
    assert not uncovered, uncovered
    # every case names family and variant, every case of the table is planned or is a column-sum case: nothing is left out
    assert all({"family", "variant"} <= set(c["plan"]["default"]) for c in PLANNED)
    assert len(PLANNED) + sum(c["entry"] == "colsum" for c in R.CASES) == len(R.CASES)
    # the exactness condition of the `ints` kind: |sum| <= 9 K (+ bias and prior contents <= 6, + column sums 3 K) stays below 2^24
    assert all(9 * c["K"] + 16 < 2 ** 24 for c in R.CASES)


@pytest.mark.parametrize("name", ["tn-split-odd-k", "lds-tt-split-xcd", "skk-kt5-nt", "tng-2-blocks-ragged", "kc-one-tile-8-splits"])
def test_ints_reference_is_the_int64_product_in_any_f32_summation_order(ops, name):
    c = R.by_name(name)
    plan = ops.gemm_plan(**R.plan_args(c))
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
