"""ops.lstm_fwd / ops.lstm_bwd on their own against the float64 reference of tests/lstm_stack_ref.py, one case per kernel variant
csrc/lstm.hip's planner can reach, judged slice by slice (per layer, gate block, 16-row batch tile, K block, third of the time axis)
so that a wrong tile cannot hide behind the tensor's largest entry.

Every case names the plan it expects (ops.lstm_plan).  The plan is asserted BEFORE anything runs: a planner change that reroutes a
shape fails here with the name of the kernel that lost its case.  Bounds: lstm_stack_ref.bound() -- 8 x the error the same
arithmetic shows on the CPU against float64, never looser than the suite's whole-tensor tolerances applied per slice; nothing in
this file is derived from what the kernels return."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lstm_stack_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

KERNELS = {      # what a plan's paths launch, for the message of a plan mismatch
    "flow": "lstm_fwd_flow2 / lstm_bwd_flow2", "big": "lstm_fwd_big / lstm_bwd_big", "big1": "lstm_fwd_big1 / lstm_bwd_big1",
    "hoist": "the hoisted lstm_bwd_step", "diag": "lstm_fwd_step / lstm_bwd_step", "diag_bf3": "lstm_fwd_step_bf3 / lstm_bwd_step_bf3"}


def _assert_plan(case, plan):
    want = case["plan"]
    got = {k: plan[k] for k in want}
    assert got == want, ("case %s was written for %s (forward) and %s (backward) with %r; the planner now answers %r -- that variant "
                         "has lost its case: give it another shape" % (case["name"], KERNELS[want["fwd_path"]], KERNELS[want["bwd_path"]], want, got))


def _run(case, inp, garbage=False):
    """One forward and backward of `case` on the GPU; everything it returns as float32 CPU tensors, plus the dropout multipliers."""
    from rnn_speech_amd import lib as _l, ops
    T, B, H, L = case["T"], case["B"], case["H"], case["L"]
    pd = "per_diagonal" in case["extras"]
    ws = ops.LstmWorkspace(T, B, H, L, precision=case["precision"])
    in_mult = out_mult = None
    if "dropout" in case["extras"]:
        ws.set_dropout(R.KEEP_IN, R.KEEP_OUT, 0x5eed0000 + T)
        in_mult = [ops.lstm_dropout_multipliers(ws, "in", l).cpu().double() for l in range(L)]
        out_mult = [ops.lstm_dropout_multipliers(ws, "out", l).cpu().double() for l in range(L)]
    _assert_plan(case, ops.lstm_plan(ws, per_diagonal=pd))
    k, b = inp["k"].cuda(), inp["b"].cuda()
    lengths = torch.as_tensor(inp["lengths"]).cuda()
    h0 = c0 = None
    if inp["h0"] is not None:
        h0, c0 = inp["h0"].cuda(), inp["c0"].cuda()
    z0, dztop = inp["z0"].clone(), inp["dztop"].clone()
    if garbage:      # finite garbage past every row's length, in the input and in the incoming gradient
        z0[inp["dead"]] = inp["garbage"][inp["dead"]]
        dztop[inp["dead"]] = -inp["garbage"][inp["dead"]]
    ws.z0.copy_(z0)
    ops.lstm_fwd(ws, k, k.stride(0), b, b.stride(0), lengths, h0, c0, per_diagonal=pd)
    ops.lstm_status(ws)
    hT, cT = ws.final_state()
    bh = B * H
    first = ws._offset(_l.WS_HFINAL) - T * bh + bh           # the h history [L][T+1][B][H]: slot t + 1 is the state after frame t
    hist = torch.as_strided(ws.buf, (L, T, B, H), ((T + 1) * bh, bh, H, 1), first)
    got = dict(ztop=ws.ztop.cpu(), h=hist.cpu(), hT=hT.cpu(), cT=cT.cpu())
    if inp["dk0"] is not None:      # lstm_bwd ACCUMULATES dK and db (amdspeech.h) and writes dz0
        dk, db = inp["dk0"].cuda(), inp["db0"].cuda()
        ws.dz0.copy_(inp["garbage"])
    else:
        dk, db = torch.zeros_like(k), torch.zeros_like(b)
    ws.dztop.copy_(dztop)
    ops.lstm_bwd(ws, k, k.stride(0), dk, db, db.stride(0), lengths, per_diagonal=pd)
    ops.lstm_status(ws)
    got.update(dK=dk.cpu(), db=db.cpu(), dz0=ws.dz0.cpu())
    for name, t in got.items():
        assert bool(torch.isfinite(t).all()), name
    return got, in_mult, out_mult


def _compare(case, got, ref, lengths, what=""):
    failures, lines = [], []
    for kind in R.OUTPUT_KINDS + R.GRAD_KINDS:
        errs = R.slice_errors(got[kind], ref[kind], kind, lengths)
        err, label = R.worst(errs)
        lim = R.bound(case, kind)
        lines.append("%-4s worst slice %.2e (bound %.1e, whole tensor %.2e)  %s" % (kind, err, lim, R.rel_err(got[kind], ref[kind]), label))
        if not err <= lim:
            bad = sorted(((e, lab) for lab, e, _ in errs if not e <= lim), reverse=True)
            failures.append("%s: %d of %d slices over %.1e, worst %s" % (kind, len(bad), len(errs), lim,
                                                                         "; ".join("%.2e %s" % x for x in bad[:6])))
    for kind in ("ztop", "dz0"):
        if not R.padding_is_zero(got[kind], lengths):
            failures.append("%s is not exactly zero at and past the rows' lengths" % kind)
    print("\n%s%s  %s/%s precision %d\n  " % (case["name"], what, R.family(case), case["regime"], case["precision"]) + "\n  ".join(lines))
    return failures


@pytest.mark.parametrize("case", R.CASES, ids=[c["name"] for c in R.CASES])
def test_stack_matches_the_float64_reference_slice_by_slice(case):
    """Padding ("padding" cases run twice, zeros and then finite garbage of magnitude 1e3 past every row's length in z0 and dztop):
    the forward results are bit-identical (tests/test_gpu_fullsize.py asserts the forward pass reproducible bit for bit) on every
    path but one: at H = 1024 in exact f32 the per-layer forward takes x . W_ih of all frames from gemm_f32, which at these small
    T * B splits K and adds the partial tiles with f32 atomics (csrc/gemm.hip, "split-K (+ f32 atomics)") -- two runs on the SAME
    input differ by ~2e-7 there, so that path's second run is held to the case's bounds like the first.  The gradients are
    compared within the case's bounds everywhere, because the weight gradients are summed with f32 atomics whose order differs
    from run to run (the same test's remark on its gradients)."""
    inp = R.make_inputs(case)
    got, in_mult, out_mult = _run(case, inp)
    ref = R.reference(case, inp, in_mult, out_mult)
    failures = _compare(case, got, ref, inp["lengths"])
    if case["precision"] == 2:
        # plain bf16 must SHOW: a case that silently ran in a higher precision is noticed.  The dataflow and per-layer kernels
        # round the recurrent operands (the outputs move); the step kernels run those in bf16x3 and only the batched products in
        # bf16 (the weight gradients move)
        kind = "dK" if R.family(case) == "diag_bf3" else "ztop"
        e = R.rel_err(got[kind], ref[kind])
        if not e > 2e-5:
            failures.append("precision 2 but %s agrees with float64 to %.1e: the call did not run in bf16" % (kind, e))
    if "padding" in case["extras"]:
        again, _, _ = _run(case, inp, garbage=True)
        atomics_in_forward = R.family(case) == "big" and case["precision"] == 0      # (see the docstring)
        for kind in () if atomics_in_forward else R.OUTPUT_KINDS:
            if not torch.equal(again[kind], got[kind]):
                failures.append("garbage past the lengths changes %s by %.2e" % (kind, float((again[kind] - got[kind]).abs().max())))
        failures += ["garbage past the lengths: " + f for f in _compare(case, again, ref, inp["lengths"], " (garbage in the padding)")]
    assert not failures, "\n".join([case["name"]] + failures)


def test_matrix_covers_every_reachable_variant():
    """The variants of csrc/lstm.hip's planner, each with the rule it comes from (lstm_stack_ref.VARIANTS), and the case(s) that
    stand for it; the plan assertion of those cases is what proves the kernel ran."""
    from rnn_speech_amd import ops
    covered = {}
    for case in R.CASES:
        for v in case["covers"]:
            covered.setdefault(v, []).append(case["name"])
    missing = sorted(set(R.VARIANTS) - set(covered))
    assert not missing, "no case for: " + "; ".join("%s (%s)" % (v, R.VARIANTS[v]) for v in missing)
    assert not set(covered) - set(R.VARIANTS)
    # what a variant's name claims, checked against the plan of every case that stands for it
    claims = {
        "diag:uw4": dict(fwd_path="diag", uw=4), "diag:uw8": dict(fwd_path="diag", uw=8), "diag:mt1": dict(fwd_path="diag", fwd_mt=1),
        "diag:mt2": dict(fwd_path="diag", fwd_mt=2), "bf3:p1": dict(fwd_path="diag_bf3", bwd_path="diag_bf3"),
        "bf3:p2": dict(fwd_path="diag_bf3", bwd_path="diag_bf3"), "bf3:H384": dict(fwd_path="diag_bf3", bwd_path="diag_bf3"),
        "hoist:H768": dict(fwd_path="diag", bwd_path="hoist"), "hoist:H1024x5": dict(fwd_path="diag", bwd_path="hoist", nmt=5),
        "flow:kb1": dict(fwd_path="flow", bwd_path="flow", kb=1), "flow:kb2": dict(fwd_path="flow", bwd_path="flow", kb=2, flow2_q=2),
        "flow:kb3": dict(fwd_path="flow", bwd_path="flow", kb=3, flow2_q=1), "flow:kb4": dict(fwd_path="flow", bwd_path="flow", kb=4, flow2_q=4),
        "flow:mv1": dict(fwd_path="flow", kb=4, mv=1, xw_parts=1), "flow:mv0-all-xcds": dict(fwd_path="flow", kb=4, mv=0, xw_parts=0),
        "flow:w8": dict(bwd_path="flow", w_pieces=8), "flow:w0": dict(bwd_path="flow", w_pieces=0),
        "flowr:kb2p1": dict(fwd_path="flow", bwd_path="flow", kb=2, flow2_q=1), "flowr:kb4p2": dict(fwd_path="flow", bwd_path="flow", kb=4, flow2_q=1),
        "flowr:kb2p2": dict(fwd_path="flow", bwd_path="flow", kb=2), "flowr:kb4p1": dict(fwd_path="flow", bwd_path="flow", kb=4),
        "big:fwd-p0": dict(fwd_path="big", pair=0), "big:fwd-p1": dict(fwd_path="big", pair=0), "big:fwd-p2": dict(fwd_path="big", pair=1),
        "big:bwd-big": dict(bwd_path="big"), "big:bwd-big1-copies": dict(bwd_path="big1", bf16p=1, bf16p_reserved=1),
        "big:copies-reserved-unused": dict(bwd_path="big", bf16p=0, bf16p_reserved=1),
        "perdiag:flow": dict(fwd_path="diag", bwd_path="diag"), "perdiag:big": dict(fwd_path="diag", bwd_path="hoist"),
    }
    by_name = {c["name"]: c for c in R.CASES}
    for v, names in covered.items():
        for name in names:
            case = by_name[name]
            ws = ops.LstmWorkspace(case["T"], case["B"], case["H"], case["L"], precision=case["precision"])
            plan = ops.lstm_plan(ws, per_diagonal="per_diagonal" in case["extras"])
            _assert_plan(case, plan)
            want = claims.get(v, {})
            assert {k: plan[k] for k in want} == want, (v, name, plan)
            if v == "flow:groups8":
                assert plan["fwd_path"] == "flow" and case["L"] * plan["nmt"] == 8
            if v == "flow:groups1":
                assert plan["fwd_path"] == "flow" and case["L"] * plan["nmt"] == 1
            if v.endswith(":long"):
                assert case["T"] >= 200
            elif v.startswith(("flowr:", "bf3:p")):
                assert case["precision"] == int(v[-1])
    # the per-diagonal request is what reroutes the two perdiag shapes
    for name, fwd in (("perdiag-flow-shape", "flow"), ("perdiag-big-shape", "big")):
        case = by_name[name]
        ws = ops.LstmWorkspace(case["T"], case["B"], case["H"], case["L"], precision=case["precision"])
        assert ops.lstm_plan(ws)["fwd_path"] == fwd


def test_plan_query_sees_the_fused_head_and_leaves_the_workspace_alone():
    from rnn_speech_amd import ops
    ws = ops.LstmWorkspace(40, 32, 512, 3)
    before = (ws.desc.flags, ws._armed, ws._fwd_seen)
    plain, head = ops.lstm_plan(ws), ops.lstm_plan(ws, head=(80, 20))
    assert plain["nfw"] == 0 and head["nfw"] > 0 and ops.lstm_ctc_fusable(ws, 80, 20)
    assert {k: v for k, v in plain.items() if k != "nfw"} == {k: v for k, v in head.items() if k != "nfw"}
    assert ops.lstm_plan(ws, head=(80, 20), per_diagonal=True)["nfw"] == 0
    assert (ws.desc.flags, ws._armed, ws._fwd_seen) == before
