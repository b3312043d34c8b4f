"""Exact-product parity of the GEMMs per kernel variant (exact f32, bf16x3, plain bf16, the packed bf16 path and its operand copies):
every case of tests/gemm_ref.py through the entry it names -- the plan first (ops.gemm_plan / ops.gemm_bf16_packed_plan must name the
kernel and the geometry the case was written for), then the operands placed as strided views into NaN-surrounded buffers, the call,
and three checks: small-integer operands bit for bit against the integer product, 0/1 selection matrices bit for bit against the
selected elements as the planned arithmetic carries them (A selecting, then B), randn operands against float64 with the criteria of
test_gpu_kernels.py; and the surroundings of every output still 7.0.  The copies: every value bit for bit against
torch.Tensor.to(torch.bfloat16).  The fallback switches (everything through the LDS kernel) are read once per process, so the cases
that name a plan for them run in a fresh child process."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gemm_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

MODE = "fallback" if os.environ.get("AMDSPEECH_GEMM_DIRECT", "1") == "0" and os.environ.get("AMDSPEECH_GEMM_KC_DIRECT", "1") == "0" else "default"
NAMES = [c["name"] for c in R.CASES if MODE in c["plan"]]      # (the column-sum cases: default mode only)


@pytest.fixture(scope="module")
def ops():
    from rnn_speech_amd import ops as o
    return o


def assert_plan(ops, c):
    plan = R.query(ops, c)
    if plan is None:
        return None
    diff = {k: (v, plan[k]) for k, v in c["plan"][MODE].items() if plan[k] != v}
    assert not diff, (c["name"], MODE, diff, plan)
    return plan


def call(ops, c, placed, scratch=None):
    v = lambda d, k: d[k].view if d.get(k) is not None else None
    d = placed[0]
    if c["entry"] == "gemm":
        fn = (ops.gemm, ops.gemm_bf16x3, ops.gemm_bf16)[c["precision"]]
        fn(v(d, "A"), v(d, "B"), trans_a=c["ta"], trans_b=c["tb"], bias=v(d, "bias"), out=v(d, "C"), accumulate=c["acc"])
    elif c["entry"] == "linear_bwd":      # (w is only read for dx, which is not asked for)
        w = torch.empty(c["M"], c["N"], device="cuda")
        ops.linear_bwd(v(d, "A"), w, v(d, "B"), v(d, "C"), v(d, "cs"), need_dx=False)
    elif c["entry"] == "tn_group":
        cs = [v(p, "cs") for p in placed]
        ops.gemm_tn_group([p["A"].view for p in placed], [p["B"].view for p in placed], [p["C"].view for p in placed],
                          colsum=cs if c["colsum"] else None, accumulate=c["acc"])
    elif c["entry"] == "packed":
        out = ops.gemm_bf16_packed(v(d, "A"), v(d, "B"), trans_a=c["ta"], trans_b=c["tb"], bias=v(d, "bias"), out=v(d, "C"), accumulate=c["acc"],
                                   scratch=scratch)
        assert out is not None, "the packed path does not take the shape of %s" % c["name"]
    elif c["entry"] in ("copy", "copy_t"):
        ops.bf16_copy(v(d, "B"), v(d, "D"), transpose=c["entry"] == "copy_t", colsum=v(d, "cs"), plain=v(d, "P"))
    elif c["entry"] == "transpose16":
        ops.bf16_transpose(v(d, "B"), v(d, "D"))
    else:
        ops.colsum_accumulate(v(d, "B"), v(d, "cs"))
    torch.cuda.synchronize()


def run_kind(ops, c, kind, plan):
    """-> (list of failures, worst rel_err of the kind, its worst absolute error)"""
    probs = R.operands(c, kind, plan)
    placed = R.place(c, probs)
    call(ops, c, placed)
    fam = plan["family"] if plan else c["entry"]
    fails, worst, worst_abs = [], 0.0, 0.0
    for i, (o, d) in enumerate(zip(probs, placed)):
        for key in ("D", "P"):      # the copies' bf16 outputs
            if d.get(key) is not None:
                got = d[key].result()
                if not np.array_equal(got, o[key]):
                    fails.append("%s %s: %s" % (kind, key, R.mismatches16(got, o[key])))
        for key, ref, exact in (("C", o.get("C"), o.get("exact")), ("cs", o.get("cs"), o.get("cs_exact"))):
            if ref is None or d.get(key) is None:
                continue
            got = d[key].result()
            tag = "%s problem %d %s" % (kind, i, key)
            if not np.isfinite(got).all():
                fails.append("%s: %d non-finite results" % (tag, int((~np.isfinite(got)).sum())))
            elif exact:
                if not R.bits_equal(got, ref):
                    fails.append("%s: %s" % (tag, R.mismatches(got, ref)))
            else:
                bound_abs, bound_rel = R.normal_bound(c, fam)
                if c["precision"] == 2 and fam in ("bf3", "bf16p") and key == "C":      # against the product of the ROUNDED operands (test_gpu_kernels.py)
                    rnd = lambda x: torch.as_tensor(x).to(torch.bfloat16).to(torch.float64).numpy()
                    A, B = rnd(o["A"].T if c["ta"] else o["A"]), rnd(o["B"].T if c["tb"] else o["B"])
                    ref = A @ B + (o["bias"] if o["bias"] is not None else 0) + (o["C0"] if o["C0"] is not None else 0)
                err = R.rel_err(got, ref)
                worst, worst_abs = max(worst, err), max(worst_abs, float(np.abs(got - ref).max()))
                if bound_rel is not None and not err < bound_rel:
                    fails.append("%s: rel_err %.3g >= %.3g" % (tag, err, bound_rel))
                if bound_abs is not None and not np.abs(got - ref).max() < bound_abs:
                    fails.append("%s: max abs err %.3g >= %.3g" % (tag, np.abs(got - ref).max(), bound_abs))
        for key in ("C", "cs", "D", "P"):
            if d.get(key) is not None and not d[key].surroundings_intact():
                fails.append("%s problem %d: the surroundings of %s were written" % (kind, i, key))
    return fails, worst, worst_abs


@pytest.mark.parametrize("name", NAMES)
def test_gemm_case(ops, name):
    c = R.by_name(name)
    plan = assert_plan(ops, c)
    fails, worst, worst_abs = [], 0.0, 0.0
    for kind in R.kinds(c):
        f, w, wa = run_kind(ops, c, kind, plan)
        fails += f
        worst, worst_abs = max(worst, w), max(worst_abs, wa)
    p = plan or dict(family=c["entry"], variant=0, splits=1, map=0)
    print("GEMMPATH %s %s/%d splits=%d map=%d normal rel_err=%.3g abs_err=%.3g" % (name, p["family"], p["variant"], p["splits"], p["map"], worst,
                                                                                   worst_abs))
    assert not fails, "%s [%s]:\n  " % (name, MODE) + "\n  ".join(fails[:12])


if MODE == "default":      # (the child process of the last test runs the cases alone)
    def test_grouped_entry_refuses_a_shape_the_kernel_does_not_take(ops):
        """Rows that are not 16-byte aligned: an error, no other kernel, nothing written."""
        from rnn_speech_amd import lib
        a = torch.zeros(64, 130, device="cuda")
        b = torch.zeros(64, 128, device="cuda")
        out = torch.full((130, 128), 7.0, device="cuda")
        with pytest.raises(lib.AmdSpeechError, match="does not qualify"):
            ops.gemm_tn_group([a, a], [b, b], [out, out.clone()])
        torch.cuda.synchronize()
        assert bool((out == 7.0).all())

    @pytest.mark.parametrize("name", [c["name"] for c in R.REFUSED])
    def test_reduced_precision_refuses_an_operand_that_is_not_16_byte_aligned(ops, name):
        """An error from the call and, with the same message, from the plan query; C and its surroundings as they were."""
        from rnn_speech_amd import lib
        c = R.by_name(name)
        with pytest.raises(lib.AmdSpeechError, match="16-byte aligned"):
            R.query(ops, c)
        probs = R.operands(c, "ints")
        placed = R.place(c, probs)
        before = placed[0]["C"].result().copy()
        with pytest.raises(lib.AmdSpeechError, match="16-byte aligned"):
            call(ops, c, placed)
        torch.cuda.synchronize()
        assert R.bits_equal(placed[0]["C"].result(), before) and placed[0]["C"].surroundings_intact()
        print("GEMMPATH %s refused" % name)

    @pytest.mark.parametrize("name", [c["name"] for c in R.NOT_TAKEN])
    def test_packed_path_does_not_take_the_shape(ops, name):
        """Scratch bytes 0, None from ops.gemm_bf16_packed, a refusal from the plan query; nothing written."""
        from rnn_speech_amd import lib
        c = R.by_name(name)
        sh = R.shapes(c)
        assert lib.load().amdspeech_gemm_bf16_packed_scratch_bytes(int(c["ta"]), int(c["tb"]), c["M"], c["N"], c["K"], sh["A"][2], sh["B"][2]) == 0
        with pytest.raises(lib.AmdSpeechError, match="shape not taken"):
            R.query(ops, c)
        d = R.place(c, R.operands(c, "ints"))[0]
        before = d["C"].result().copy()
        assert ops.gemm_bf16_packed(d["A"].view, d["B"].view, trans_a=c["ta"], trans_b=c["tb"], out=d["C"].view) is None
        torch.cuda.synchronize()
        assert R.bits_equal(d["C"].result(), before) and d["C"].surroundings_intact()
        print("GEMMPATH %s not taken" % name)

    def test_packed_path_stays_inside_the_scratch_it_is_given(ops):
        """The caller's scratch: a 256-byte aligned view of exactly scratch_bytes inside a larger buffer of 0xA5; the copies and the
        split-K partial tiles all live in it, the product is exact, the bytes around the view are as they were."""
        from rnn_speech_amd import lib
        c = R.by_name(R.SCRATCH_CASE)
        plan = assert_plan(ops, c)
        assert plan["splits"] > 1
        sh = R.shapes(c)
        n = lib.load().amdspeech_gemm_bf16_packed_scratch_bytes(int(c["ta"]), int(c["tb"]), c["M"], c["N"], c["K"], sh["A"][2], sh["B"][2])
        assert n > 0
        buf = torch.full((n + 1024,), 0xA5, dtype=torch.uint8, device="cuda")
        start = 256 + (-(buf.data_ptr() + 256)) % 256
        view = buf[start:start + n]
        assert view.data_ptr() % 256 == 0 and start >= 256 and start + n + 256 <= buf.numel()
        probs = R.operands(c, "ints", plan)
        placed = R.place(c, probs)
        call(ops, c, placed, scratch=view)
        got = placed[0]["C"].result()
        assert R.bits_equal(got, probs[0]["C"]), R.mismatches(got, probs[0]["C"])
        assert placed[0]["C"].surroundings_intact()
        host = buf.cpu()
        assert bool((host[:start] == 0xA5).all()) and bool((host[start + n:] == 0xA5).all())
        assert not bool((host[start:start + n] == 0xA5).all())      # (and the view was used)
        with pytest.raises(ValueError, match="scratch"):
            call(ops, c, placed, scratch=buf[start:start + n - 1])
        print("GEMMPATH %s scratch view of %d bytes" % (c["name"], n))

    def test_gemm_cases_under_the_fallback_switches():
        """The cases that name a plan for AMDSPEECH_GEMM_DIRECT=0 AMDSPEECH_GEMM_KC_DIRECT=0 (the LDS kernel at the LDS-free kernels'
        shapes), in a fresh child process with its own time limit."""
        out = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-m", "gpu", "-q", "-s", "-k", "test_gemm_case"],
                             env=dict(os.environ, **R.FALLBACK_ENV), capture_output=True, text=True, timeout=600)
        for line in out.stdout.splitlines():
            if "GEMMPATH" in line:
                print(line[line.index("GEMMPATH"):], "[fallback]")
        assert out.returncode == 0, out.stdout[-4000:] + out.stderr[-2000:]
        n = sum(1 for c in R.CASES if "fallback" in c["plan"])
        assert out.stdout.count("GEMMPATH ") == n, (n, out.stdout[-2000:])
