"""Exact-product parity of the f32 GEMM per kernel variant: every case of tests/gemm_ref.py through the entry it names -- the plan first
(ops.gemm_plan must name the kernel and the geometry the case was written for), then the operands placed as strided views into
NaN-surrounded buffers, the call, and three checks: small-integer operands bit for bit against the integer product, 0/1 selection
matrices bit for bit against the selected elements (A selecting, then B), randn operands against float64 with the criterion of
test_gpu_kernels.py; and the surroundings of every output still 7.0.  The fallback switches (everything through the LDS kernel)
are read once per process, so the cases that name a plan for them run in a fresh child process."""
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
    if c["entry"] == "colsum":
        return None
    plan = ops.gemm_plan(**R.plan_args(c))
    diff = {k: (v, plan[k]) for k, v in c["plan"][MODE].items() if plan[k] != v}
    assert not diff, (c["name"], MODE, diff, plan)
    return plan


def call(ops, c, placed):
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
    else:
        ops.colsum_accumulate(v(d, "B"), v(d, "cs"))
    torch.cuda.synchronize()


def run_kind(ops, c, kind, plan):
    """-> (list of failures, worst rel_err of the kind)"""
    probs = R.operands(c, kind, plan)
    placed = R.place(c, probs)
    call(ops, c, placed)
    fam = plan["family"] if plan else "colsum"
    fails, worst = [], 0.0
    for i, (o, d) in enumerate(zip(probs, placed)):
        for key, ref, exact in (("C", o.get("C"), o.get("exact")), ("cs", o.get("cs"), o.get("cs_exact"))):
            if ref is None or d.get(key) is None:
                continue
            got = d[key].result()
            tag = "%s problem %d %s" % (kind, i, key)
            if not np.isfinite(got).all():
                fails.append("%s: %d non-finite results" % (tag, int((~np.isfinite(got)).sum())))
            elif exact and fam == "bf3" and kind in ("selA", "selB"):
                # a bf16 pair carries 16 bits, one bf16 8: the probe must SEE the arithmetic (and still be close)
                if R.bits_equal(got, ref):
                    fails.append("%s: reduced precision returned all 24 bits" % tag)
                if R.rel_err(got, ref) > 2.0 ** -8:      # (rounding to 8 significant bits: half an ulp, 2^-9 of the element)
                    fails.append("%s: rel_err %.3g" % (tag, R.rel_err(got, ref)))
            elif exact:
                if not R.bits_equal(got, ref):
                    fails.append("%s: %s" % (tag, R.mismatches(got, ref)))
            else:
                bound_abs, bound_rel = R.normal_bound(c, fam)
                if c["precision"] == 2 and fam == "bf3" and key == "C":      # against the product of the ROUNDED operands (test_gpu_kernels.py)
                    rnd = lambda x: torch.as_tensor(x).to(torch.bfloat16).to(torch.float64).numpy()
                    A, B = rnd(o["A"].T if c["ta"] else o["A"]), rnd(o["B"].T if c["tb"] else o["B"])
                    ref = A @ B + (o["bias"] if o["bias"] is not None else 0) + (o["C0"] if o["C0"] is not None else 0)
                err = R.rel_err(got, ref)
                worst = max(worst, err)
                if bound_rel is not None and not err < bound_rel:
                    fails.append("%s: rel_err %.3g >= %.3g" % (tag, err, bound_rel))
                if bound_abs is not None and not np.abs(got - ref).max() < bound_abs:
                    fails.append("%s: max abs err %.3g >= %.3g" % (tag, np.abs(got - ref).max(), bound_abs))
        for key in ("C", "cs"):
            if d.get(key) is not None and not d[key].surroundings_intact():
                fails.append("%s problem %d: the surroundings of %s were written" % (kind, i, key))
    return fails, worst


@pytest.mark.parametrize("name", NAMES)
def test_gemm_case(ops, name):
    c = R.by_name(name)
    plan = assert_plan(ops, c)
    fails, worst = [], 0.0
    for kind in R.kinds(c):
        f, w = run_kind(ops, c, kind, plan)
        fails += f
        worst = max(worst, w)
    p = plan or dict(family="colsum", variant=0, splits=1, map=0)
    print("GEMMPATH %s %s/%d splits=%d map=%d normal rel_err=%.3g" % (name, p["family"], p["variant"], p["splits"], p["map"], worst))
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
