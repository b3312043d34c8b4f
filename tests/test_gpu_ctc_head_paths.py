"""The CTC head inside the whole-sequence LSTM launches (ops.lstm_fwd(..., head=) / ops.lstm_bwd(..., head=): ctc_follower and
ctc_leader of csrc/ctc_flow.h) against float64, stage by stage and slice by slice, one case per thing the head's code does
differently from shape to shape (tests/ctc_head_ref.py: the cases, the stage references, the bounds -- none of them taken from what
the kernels return).

Every case names the plan it expects (ops.lstm_plan with the head); the plan is asserted BEFORE anything runs, so a planner change
names the variant that lost its case.  logits, dlogits and loss live as contiguous views inside larger tensors pre-filled with a
NaN pattern: two guard frames before and after, guard entries around the loss; the guards must come back bit-identical."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ctc_head_ref as R  # noqa: E402
import lstm_stack_ref as S  # noqa: E402

pytestmark = pytest.mark.gpu


def _assert_plan(case, plan):
    want = case["plan"]
    got = {k: plan[k] for k in want}
    assert got == want, ("case %s stands for %s with the plan %r; the planner now answers %r -- those variants have lost their case: "
                         "give them another shape" % (case["name"], ", ".join(case["covers"]), want, got))


def _guarded(lead, shape, tail):
    """(raw int32 tensor, float32 view of `shape` inside it): `lead` / `tail` guard elements around the view, all NaN-patterned."""
    n = int(np.prod(shape))
    raw = torch.full((lead + n + tail,), R.PATTERN, dtype=torch.int32, device="cuda")
    return raw, raw.view(torch.float32)[lead:lead + n].view(*shape)


def _guards_intact(raw, lead, n):
    return bool((raw[:lead] == R.PATTERN).all()) and bool((raw[lead + n:] == R.PATTERN).all())


def _mini_batch(case, ws, cws, inp, training, failures):
    """One forward and one backward call with the head on `ws`; everything read back as float32 CPU tensors."""
    from rnn_speech_amd import lib as _l, ops
    T, B, H, L, C = inp["T"], case["B"], case["H"], case["L"], case["C"]
    in_mult = out_mult = None
    if "dropout" in case["extras"]:
        ws.set_dropout(S.KEEP_IN, S.KEEP_OUT, 0x5eed0000 + T)
        in_mult = [ops.lstm_dropout_multipliers(ws, "in", l).cpu().double() for l in range(L)]
        out_mult = [ops.lstm_dropout_multipliers(ws, "out", l).cpu().double() for l in range(L)]
    k, b = inp["k"].cuda(), inp["b"].cuda()
    lengths, dense = torch.as_tensor(inp["lengths"]).cuda(), torch.as_tensor(inp["dense"]).cuda()
    wo, bo = inp["wo"].cuda(), inp["bo"].cuda()
    frame = B * C
    raw_lg, logits = _guarded(2 * frame, (T, B, C), 2 * frame)
    raw_dl, dlogits = _guarded(2 * frame, (T, B, C), 2 * frame)
    raw_ls, loss = _guarded(8, (B,), 8)
    head = ops.CtcHead(wo, bo, logits, dense, loss, dlogits, cws)
    h0 = c0 = None
    if inp["h0"] is not None:
        h0, c0 = inp["h0"].cuda(), inp["c0"].cuda()
    ws.z0.copy_(inp["z0"])
    ops.lstm_fwd(ws, k, k.stride(0), b, b.stride(0), lengths, h0, c0, training=training, head=head)
    ops.lstm_status(ws)
    hT, cT = ws.final_state()
    bh = B * H
    first = ws._offset(_l.WS_HFINAL) - T * bh + bh           # the h history [L][T+1][B][H]: slot t + 1 is the state after frame t
    hist = torch.as_strided(ws.buf, (L, T, B, H), ((T + 1) * bh, bh, H, 1), first)
    got = dict(ztop=ws.ztop.cpu(), h=hist.cpu(), hT=hT.cpu(), cT=cT.cpu(), logits=logits.cpu(), loss=loss.cpu())
    if inp["dk0"] is not None:      # lstm_bwd ACCUMULATES dK and db and writes dz0
        dk, db = inp["dk0"].cuda(), inp["db0"].cuda()
        ws.dz0.copy_(inp["garbage"])
    else:
        dk, db = torch.zeros_like(k), torch.zeros_like(b)
    ops.lstm_bwd(ws, k, k.stride(0), dk, db, db.stride(0), lengths, head=head)
    ops.lstm_status(ws)
    got.update(dlogits=dlogits.cpu(), dztop=ws.dztop.cpu(), dK=dk.cpu(), db=db.cpu(), dz0=ws.dz0.cpu())
    if not torch.equal(got["logits"], logits.cpu()) or not torch.equal(got["loss"], loss.cpu()):
        failures.append("the backward call changed the logits or the loss")
    for name, raw, lead, n in (("logits", raw_lg, 2 * frame, T * frame), ("dlogits", raw_dl, 2 * frame, T * frame), ("loss", raw_ls, 8, B)):
        if not _guards_intact(raw, lead, n):
            failures.append("the guard entries around %s were written" % name)
    for name, t in got.items():
        if not bool(torch.isfinite(t).all()):
            failures.append("%s is not finite (an entry never written keeps the NaN pattern)" % name)
    return got, in_mult, out_mult


def _run(case, failures):
    from rnn_speech_amd import ops
    B, H, L, C, U = case["B"], case["H"], case["L"], case["C"], case["U"]
    root = ops.LstmWorkspace(case["alloc_T"], B, H, L, precision=case["precision"])
    cws = ops.CtcWorkspace(case["alloc_T"], B, C, U)
    ws = root.prefix(case["T"])
    assert (ws is not root) == (case["alloc_T"] > case["T"])
    assert ops.lstm_ctc_fusable(ws, C, U)
    plan = ops.lstm_plan(ws, head=(C, U))
    _assert_plan(case, plan)
    assert plan["nfw"] > 0 and R.teams(case, plan) == R.teams(case)
    second = "second" in case["extras"]
    if second:      # the first mini-batch of the pair: the whole allocation, training=True arms the panels of the next call
        first = R.make_inputs(case, case["first_T"])
        _assert_plan(dict(case, plan=dict(case["plan"], w_pieces=8 if case["first_T"] >= 64 else 0)), ops.lstm_plan(root, head=(C, U)))
        _mini_batch(case, root, cws, first, True, failures)
    inp = R.make_inputs(case)
    got, in_mult, out_mult = _mini_batch(case, ws, cws, inp, second, failures)
    return inp, got, in_mult, out_mult


@pytest.mark.parametrize("case", R.CASES, ids=[c["name"] for c in R.CASES])
def test_head_matches_float64_stage_by_stage(case):
    failures = []
    inp, got, in_mult, out_mult = _run(case, failures)
    fails, ratios, lines = R.judge(case, inp, got, in_mult, out_mult)
    print("\nHEADPATH %s  %s  precision %d  UPT %d\n  " % (case["name"], case["regime"], case["precision"], R.upt(case)) + "\n  ".join(lines))
    print("HEADRATIO %s %s" % (case["name"], " ".join("%d:%.3f" % (s, ratios[s]) for s in sorted(ratios))))
    if case["precision"] == 2:      # plain bf16 must SHOW (tests/test_gpu_lstm_stack.py): a silent run in a higher precision is noticed
        f = S.forward(inp["z0"], inp["k"], inp["b"], inp["lengths"], inp["h0"], inp["c0"])
        e = S.rel_err(got["ztop"], f["ztop"])
        if not e > 2e-5:
            failures.append("precision 2 but ztop agrees with float64 to %.1e: the call did not run in bf16" % e)
    failures += fails
    assert not failures, "\n".join([case["name"]] + failures)


def test_table_covers_every_variant_and_the_plans_bear_the_names_out():
    from rnn_speech_amd import ops
    covered = {}
    for case in R.CASES:
        for v in case["covers"]:
            covered.setdefault(v, []).append(case)
    missing = sorted(set(R.VARIANTS) - set(covered))
    assert not missing, "no case for: " + "; ".join("%s (%s)" % (v, R.VARIANTS[v]) for v in missing)
    assert not set(covered) - set(R.VARIANTS)
    claims = {"kb1": dict(kb=1), "kb2": dict(kb=2), "kb3": dict(kb=3), "kb4-xw": dict(kb=4, mv=1), "w8": dict(w_pieces=8),
              "w0-T63": dict(w_pieces=0), "T64": dict(w_pieces=8), "T65": dict(w_pieces=8)}
    for v, cases in covered.items():
        for case in cases:
            ws = ops.LstmWorkspace(case["alloc_T"], case["B"], case["H"], case["L"], precision=case["precision"]).prefix(case["T"])
            plan = ops.lstm_plan(ws, head=(case["C"], case["U"]))
            _assert_plan(case, plan)
            assert plan["fwd_path"] == "flow" and plan["bwd_path"] == "flow" and plan["nfw"] > 0
            want = claims.get(v, {})
            assert {k: plan[k] for k in want} == want, (v, case["name"], plan)
            nteams, B = R.teams(case, plan), case["B"]
            if v == "upt2-cap":
                assert R.upt(case, plan) == 2 and B == 2 * nteams
            if v == "upt2-unreal":
                assert R.upt(case, plan) == 2 and nteams < B < 2 * nteams - 1
            if v == "upt1-edge":
                assert R.upt(case, plan) == 1 and B == nteams
            if v == "upt2-edge":
                assert R.upt(case, plan) == 2 and B == nteams + 1
            if v in ("bf16x3", "bf16"):
                assert case["precision"] == {"bf16x3": 1, "bf16": 2}[v]
            if v.startswith("C") and v[1:].isdigit():
                assert case["C"] == int(v[1:])


@pytest.mark.parametrize("what,L,H,B,T,C,U", R.REFUSALS, ids=[r[0] for r in R.REFUSALS])
def test_shapes_the_head_refuses_raise_and_write_nothing(what, L, H, B, T, C, U):
    from rnn_speech_amd import lib as _l, ops
    ws = ops.LstmWorkspace(T, B, H, L)
    assert not ops.lstm_ctc_fusable(ws, C, U)
    assert ops.lstm_plan(ws, head=(C, U))["nfw"] == 0
    g = torch.Generator(device="cpu").manual_seed(3)
    k, b = (torch.randn(L, 2 * H, 4 * H, generator=g) * 0.05).cuda(), torch.zeros(L, 4 * H).cuda()
    wo, bo = (torch.randn(H, C, generator=g) * 0.1).cuda(), torch.zeros(C).cuda()
    lengths = torch.full((B,), T, dtype=torch.int32).cuda()
    dense = torch.ones(B, U, dtype=torch.int32).cuda()
    raw_lg, logits = _guarded(2 * B * C, (T, B, C), 2 * B * C)
    raw_dl, dlogits = _guarded(2 * B * C, (T, B, C), 2 * B * C)
    raw_ls, loss = _guarded(8, (B,), 8)
    head = ops.CtcHead(wo, bo, logits, dense, loss, dlogits, ops.CtcWorkspace(T, B, C, U))
    ws.z0.copy_(torch.randn(T, B, H, generator=g))
    with pytest.raises(_l.AmdSpeechError):
        ops.lstm_fwd(ws, k, k.stride(0), b, b.stride(0), lengths, None, None, head=head)
    torch.cuda.synchronize()
    for raw in (raw_lg, raw_dl, raw_ls):      # guards AND the outputs themselves: nothing was written
        assert bool((raw == R.PATTERN).all()), what
