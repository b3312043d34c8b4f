"""ops.lstm_bidir_fwd / ops.lstm_bidir_bwd on their own -- no Engine, no Linear layers, no CTC -- against the float64 reference of
tests/bidir_layer_ref.py, one case per kernel variant, launch path and edge of the layer-wise bidirectional driver (csrc/lstm_bidir.h),
judged slice by slice (layer, direction, gate block, 16 batch rows, 16 hidden units, third of the frames, x / h rows of a kernel
gradient) so that a wrong tile cannot hide behind a tensor's largest entry.

Every case names the launch path it expects on an MI355X; that path and the whole plan of the call (amdspeech_lstm_bidir_plan against
bidir_layer_ref.expected_plan: kernel variant and launch geometry of both passes) are asserted BEFORE anything runs.
Bounds: bidir_layer_ref.bound() -- 8 x the error the same arithmetic shows on the CPU against float64, never looser than the suite's
whole-tensor tolerances applied per slice; nothing in this file is derived from what the kernels return."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bidir_layer_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

LAUNCHES = {2: "one persistent launch for both directions", 1: "one persistent launch per direction", 0: "one launch per frame"}


def _assert_path(case, ws):
    """The library's plan for the case (amdspeech_lstm_bidir_plan) is the mirror's, field by field -- kernel variant, waves, row
    groups, workgroups and LDS of both passes, on 256 CUs -- so what `covers` names is what runs; nothing is launched here."""
    from rnn_speech_amd import ops
    plan, got, want = ops.lstm_bidir_plan(ws), ws.path(), case["path"]
    assert plan["path"] == got and plan["cus"] == 256, plan
    if "per_frame" in case["extras"]:
        # (the flag, not the plan, sends this case to the per-frame launches: without it the plan is that of the bare shape, and what
        #  it says is reported)
        flagged, bare = ops.lstm_bidir_plan(ws, per_frame=True), dict(case, extras=())
        assert flagged["path"] == 0 and flagged == R.expected_plan(case), (case["name"], flagged, R.expected_plan(case))
        assert plan == R.expected_plan(bare), (case["name"], plan, R.expected_plan(bare))
        return got
    assert got == want, ("case %s was written for %s (path %d); amdspeech_lstm_bidir_path now answers %d (%s) -- that variant has lost "
                         "its case: give it another shape" % (case["name"], LAUNCHES[want], want, got, LAUNCHES.get(got, "?")))
    assert plan == R.expected_plan(case), (case["name"], plan, R.expected_plan(case))
    return got


def _run(case, inp, garbage=False, per_frame=None):
    """One forward and backward of `case` on the GPU; everything it returns as float32 CPU tensors, plus the dropout multipliers."""
    from rnn_speech_amd import ops
    T, B, H, L = case["T"], case["B"], case["H"], case["L"]
    pf = ("per_frame" in case["extras"]) if per_frame is None else per_frame
    ws = ops.BidirWorkspace(T, B, H, L, precision=case["precision"])
    masks = None
    if "dropout" in case["extras"]:
        ws.set_dropout(R.KEEP_IN, R.KEEP_OUT, 0x5eed0000 + T)
        masks = {(d, w, l): ops.lstm_bidir_dropout_multipliers(ws, d, w, l).cpu().double()
                 for d in R.DIRS for w in ("in", "out") for l in range(L)}
    planned = _assert_path(case, ws)
    ks, bs = [k.cuda() for k in inp["ks"]], [b.cuda() for b in inp["bs"]]
    lengths = torch.as_tensor(inp["lengths"]).cuda()
    h0 = c0 = None
    if inp["h0"] is not None:
        h0, c0 = inp["h0"].cuda(), inp["c0"].cuda()
    z0, dyf, dyb = inp["z0"].clone(), inp["dytop_fw"].clone(), inp["dytop_bw"].clone()
    if garbage:      # finite values of magnitude 1e3 past every row's length, in the input and in both incoming gradients
        dead = inp["dead"]
        z0[dead], dyf[dead], dyb[dead] = inp["garbage"][dead], -inp["garbage"][dead], inp["garbage"].flip(2)[dead]
    ws.z0.copy_(z0)
    ops.lstm_bidir_fwd(ws, ks, bs, lengths, h0, c0, per_frame=pf)
    ops.lstm_bidir_status(ws)
    y_fw, y_bw = ws.layer_outputs()
    assert torch.equal(y_fw[L - 1], ws.ytop_fw) and torch.equal(y_bw[L - 1], ws.ytop_bw)
    hT, cT = ws.final_state()
    got = dict(y=torch.stack([y_fw, y_bw], dim=1).cpu(), hT=hT.cpu(), cT=cT.cpu())
    if inp["dk0"] is not None:      # lstm_bidir_bwd ACCUMULATES dK and db (amdspeech.h) and writes dz0
        dks, dbs = [t.cuda() for t in inp["dk0"]], [t.cuda() for t in inp["db0"]]
        ws.dz0.copy_(inp["garbage"])
    else:
        dks, dbs = [torch.zeros_like(k) for k in ks], [torch.zeros_like(b) for b in bs]
    ws.dytop_fw.copy_(dyf)
    ws.dytop_bw.copy_(dyb)
    ops.lstm_bidir_bwd(ws, ks, dks, dbs, lengths, per_frame=pf)
    ops.lstm_bidir_status(ws)
    got.update(dK=[t.cpu() for t in dks], db=[t.cpu() for t in dbs], dz0=ws.dz0.cpu())
    for name, t in got.items():
        for x in (t if isinstance(t, list) else [t]):
            assert bool(torch.isfinite(x).all()), name
    return got, masks, planned


def _compare(case, got, ref, info):
    failures, lines = [], []
    for kind in R.KINDS:
        errs = R.slice_errors(got[kind], ref[kind], kind, info)
        err, label = R.worst(errs)
        lim = R.bound(case, kind)
        lines.append("%-3s worst slice %.2e (bound %.1e%s, whole tensor %.2e)  %s" % (kind, err, lim, ", within 2x" if err > lim / 2 else "",
                                                                                    R.whole_errors(got[kind], ref[kind], kind), label))
        if not err <= lim:
            bad = sorted(((e, lab) for lab, e, _ in errs if not e <= lim), reverse=True)
            failures.append("%s: %d of %d slices over %.1e, worst %s" % (kind, len(bad), len(errs), lim,
                                                                         "; ".join("%.2e %s" % x for x in bad[:6])))
    for kind in ("y", "dz0"):
        if not R.padding_is_zero(got[kind], info["lengths"]):
            failures.append("%s is not exactly zero at and past the rows' lengths" % kind)
    return failures, lines


def _report(case, planned, pf, lines, what=""):
    print("\n%s%s  precision %d/%s  path %s\n  " % (case["name"], what, case["precision"], case["regime"],
                                                   "0 by the flag (the plan: %d)" % planned if pf else "%d by the plan" % planned) + "\n  ".join(lines))


@pytest.mark.parametrize("case", R.CASES, ids=[c["name"] for c in R.CASES])
def test_bidir_calls_match_the_float64_reference_slice_by_slice(case):
    """"padding" cases run twice: zeros, then finite values of magnitude 1e3 past every row's length in z0 and both dytop.  The
    forward results must be bit-identical (nothing of the forward pass sums in an order that changes from run to run at these
    shapes: the batched product x . W_ih splits K only from K = 512 on, csrc/gemm.hip); the gradients are compared within the case's
    bounds, because the weight gradients are summed with f32 atomics."""
    inp = R.make_inputs(case)
    info = R.info_of(case, inp["lengths"])
    got, masks, planned = _run(case, inp)
    ref = R.reference(case, inp, masks)
    failures, lines = _compare(case, got, ref, info)
    _report(case, planned, "per_frame" in case["extras"], lines)
    if "padding" in case["extras"]:
        again, _, _ = _run(case, inp, garbage=True)
        for kind in R.OUTPUT_KINDS:
            if not torch.equal(again[kind], got[kind]):
                failures.append("values past the lengths change %s by %.2e" % (kind, float((again[kind] - got[kind]).abs().max())))
        f2, lines = _compare(case, again, ref, info)
        _report(case, planned, False, lines, " (1e3 past the lengths)")
        failures += ["values past the lengths: " + f for f in f2]
    assert not failures, "\n".join([case["name"]] + failures)


def test_matrix_reaches_every_variant_and_every_launch_path():
    """Every VARIANTS entry has a case, and over the matrix this device's plan answers 2, 1 and 0, with 0 by the flag besides."""
    from rnn_speech_amd import ops
    covered = {v for c in R.CASES for v in c["covers"]}
    missing = sorted(set(R.VARIANTS) - covered)
    assert not missing, "no case for: " + "; ".join("%s (%s)" % (v, R.VARIANTS[v]) for v in missing)
    assert not covered - set(R.VARIANTS)
    by_plan, by_flag = {}, []
    for case in R.CASES:
        ws = ops.BidirWorkspace(case["T"], case["B"], case["H"], case["L"], precision=case["precision"])
        planned = _assert_path(case, ws)
        if "per_frame" in case["extras"]:
            assert planned != 0, "%s: the plan already answers 0 for this shape, so the flag is not what is tested" % case["name"]
            by_flag.append(case["name"])
        else:
            by_plan.setdefault(planned, []).append(case["name"])
        del ws
    print("\npaths by the plan: " + "; ".join("%d: %d cases (%s ...)" % (p, len(n), n[0]) for p, n in sorted(by_plan.items())) +
          "\npath 0 by the flag: " + ", ".join(by_flag))
    assert set(by_plan) == {0, 1, 2}, by_plan
    assert {c["precision"] for c in R.CASES if c["name"] in by_flag} == {0, 1}, by_flag


def test_per_frame_and_persistent_launches_agree_with_float64_alike():
    """The same bf16x3 shape with per_frame=True and on its planned persistent path: both within the same bounds of float64.  (Bit
    equality is not demanded: the weight gradients are summed with atomics, and nothing in amdspeech.h promises it.)"""
    case = next(c for c in R.CASES if c["name"] == "bf3-per-frame")
    inp = R.make_inputs(case)
    info = R.info_of(case, inp["lengths"])
    ref = R.reference(case, inp, None)
    failures = []
    for pf in (True, False):
        got, _, planned = _run(case, inp, per_frame=pf)
        assert planned in (1, 2), "the planned path of %s is per-frame already" % case["name"]
        f, lines = _compare(case, got, ref, info)
        _report(case, planned, pf, lines)
        failures += ["per_frame=%r: %s" % (pf, x) for x in f]
    assert not failures, "\n".join(failures)
