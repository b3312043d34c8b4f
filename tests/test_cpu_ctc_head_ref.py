"""tests/ctc_head_ref.py tied down without a GPU: the emulated arithmetic passes its own bounds, the slices catch five planted
mistakes that the older whole-tensor tolerances let through, the case table covers what it claims (VARIANTS, the UPT arithmetic,
the refusals), no slice is left out beyond the stated rule, and every label row fits its frames."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ctc_head_ref as R  # noqa: E402
import ctc_ref as CR  # noqa: E402
import lstm_stack_ref as S  # noqa: E402

IDS = [c["name"] for c in R.CASES]


# ------------------------------------------------------------------------------------------------ 1: the emulation under its bounds
@pytest.mark.parametrize("case", R.CASES, ids=IDS)
def test_emulated_arithmetic_passes_its_own_bounds_with_margin(case):
    """Every stage at half its bound or less -- but where a bound of stage 1 or 5 IS lstm_stack_ref's cap (plain bf16: 8 x the
    emulation's error is over today's whole-tensor tolerance), the arithmetic of the precision itself sits near it, as in the stack
    matrix; there the emulation only has to pass."""
    inp, (im, om), got = R.emulated(case["name"])
    fails, ratios, lines = R.judge(case, inp, got, im, om)
    assert not fails, "\n".join(fails)
    for stage in (1, 2, 3, 4, 5):
        kinds = {1: S.OUTPUT_KINDS, 5: S.GRAD_KINDS}.get(stage, ())
        capped = any(R.bound(case, k) == S.CAPS[case["precision"]][0 if k in S.OUTPUT_KINDS else 1] for k in kinds)
        assert ratios[stage] <= (1.0 if capped else 0.5), (stage, ratios, lines)
    assert case["precision"] == 2 or not any(R.bound(case, k) == S.CAPS[case["precision"]][0 if k in S.OUTPUT_KINDS else 1]
                                             for k in S.OUTPUT_KINDS + S.GRAD_KINDS)


def test_recorded_tables_are_the_emulated_arithmetic_of_this_table():
    """The tables in ctc_head_ref.py are a recorded run; float32 on another CPU sums in another order, so the figures move a
    little -- but a table that no longer belongs to the cases is off by more than 4x."""
    table, lin, dzt = R.measure()
    assert set(table) == set(R.MEASURED) and set(lin) == set(R.LINEAR_MEASURED) and set(dzt) == set(R.DZTOP_MEASURED)
    for key, row in table.items():
        for kind, e in row.items():
            assert R.MEASURED[key][kind] / 4 <= e <= 4 * R.MEASURED[key][kind], (key, kind, e)
    for now, rec in ((lin, R.LINEAR_MEASURED), (dzt, R.DZTOP_MEASURED)):
        for key, e in now.items():
            assert rec[key] / 4 <= e <= 4 * rec[key], (key, e)
    for case in R.CASES:
        for kind in S.OUTPUT_KINDS + S.GRAD_KINDS:
            assert 0 < R.bound(case, kind) <= S.CAPS[case["precision"]][0 if kind in S.OUTPUT_KINDS else 1]
        assert 0 < R.linear_bound(case) <= R.LOGIT_CAP and 0 < R.dztop_bound(case) <= R.DZTOP_CAP


# ------------------------------------------------------------------------------------------------ 2: the checker can fail
def _linear_caught(case, fault):
    inp, _, got = R.emulated(case["name"])
    bad = R.emulate_linear(got["ztop"], inp["wo"], inp["bo"], fault=fault, nteams=R.teams(case))
    ref = R.linear_ref(got["ztop"], inp["wo"], inp["bo"])
    errs = R.linear_slice_errors(bad, ref, inp["lengths"])
    return [x for x in errs if not x[1] <= R.linear_bound(case)], len(errs)


def _dztop_caught(case, fault):
    inp, _, got = R.emulated(case["name"])
    valid = [v for v, _, _ in R.row_facts(inp["dense"], inp["lengths"], case["C"])]
    bad = R.emulate_dztop(got["dlogits"], inp["wo"], fault=fault)
    ref = R.dztop_ref(got["dlogits"], inp["wo"])
    errs = R.dztop_slice_errors(bad, ref, got["dlogits"], inp["wo"], inp["lengths"], valid)
    return [x for x in errs if not x[1] <= R.dztop_bound(case)], len(errs)


def _applies(case, fault):
    return {"drop_k": True, "second_tile": R.upt(case) == 2, "clamp_last": case["T"] % 16 != 0 and case["T"] > 16,
            "neighbour_tile": True, "ignore_64": case["C"] > 64}[fault]


@pytest.mark.parametrize("fault", R.LINEAR_FAULTS + R.DZTOP_FAULTS)
def test_every_planted_mistake_is_caught_by_a_slice_in_every_case_it_applies_to(fault):
    cases = [c for c in R.CASES if _applies(c, fault)]
    assert len(cases) >= 3, fault
    for case in cases:
        bad, n = (_linear_caught if fault in R.LINEAR_FAULTS else _dztop_caught)(case, fault)
        assert bad, (fault, case["name"])
        if fault in ("second_tile", "clamp_last", "neighbour_tile"):      # a local mistake: most slices stay clean, the culprit is named
            assert len(bad) < n, (fault, case["name"])
    if fault == "neighbour_tile":
        bad, _ = _dztop_caught(cases[0], fault)
        assert all(lab.startswith("row 0 ") and lab.endswith("units 16:32") for lab, _, _ in bad)


def _quiet_linear_scene():
    """A mini-batch whose logits tensor has one large entry per frame -- class 79 carries a bias of 3e5 -- so that 2e-6 x the
    tensor's maximum is 0.6: the older whole-tensor tolerance then waves through ANY mistake in the other label tiles, whose own
    entries are of magnitude 1."""
    rng = np.random.RandomState(5)
    T, B, H, C = 33, 4, 128, 80
    ztop = (rng.randn(T, B, H) * 0.3).astype(np.float32)
    wo = (rng.randn(H, C) * 0.02).astype(np.float32)
    bo = (rng.randn(C) * 0.5).astype(np.float32)
    bo[79] = 3e5
    return ztop, wo, bo, np.array([33, 30, 33, 17], np.int32), dict(H=H, C=C)


@pytest.mark.parametrize("fault", R.LINEAR_FAULTS)
def test_logit_mistakes_pass_the_older_whole_tensor_tolerance_and_fail_the_slices(fault):
    ztop, wo, bo, lengths, shape = _quiet_linear_scene()
    ref = R.linear_ref(ztop, wo, bo)
    good, bad = R.emulate_linear(ztop, wo, bo), R.emulate_linear(ztop, wo, bo, fault=fault, nteams=2)
    old = lambda x: np.abs(x - ref).max() < R.LOGIT_CAP * max(np.abs(ref).max(), 1.0)      # tests/test_gpu_ctc_head.py's metric
    assert old(good) and old(bad), fault
    lim = R.linear_bound(shape)
    assert max(x[1] for x in R.linear_slice_errors(good, ref, lengths)) <= lim
    caught = [x for x in R.linear_slice_errors(bad, ref, lengths) if not x[1] <= lim]
    assert caught and all(not lab.endswith("labels 64:80") for lab, _, _ in caught), fault


@pytest.mark.parametrize("fault", R.DZTOP_FAULTS)
def test_dztop_mistakes_pass_the_older_whole_tensor_tolerance_and_fail_the_slices(fault):
    """A mini-batch in which the part the mistake touches has a small gradient (utterance 0 is nearly converged; the labels from 64
    on hardly occur): 5e-4 x the tensor's maximum -- the older tolerance on everything behind dlogits -- does not see it."""
    rng = np.random.RandomState(6)
    T, B, H, C = 20, 4, 128, 80
    d = (rng.randn(T, B, C) * 0.1).astype(np.float32)
    if fault == "neighbour_tile":
        d[:, 0] *= 1e-4
    else:
        d[:, :, 64:] *= 1e-4
    wo = (rng.randn(H, C) * 0.35).astype(np.float32)
    lengths, valid = np.full(B, T, np.int32), [True] * B
    ref = R.dztop_ref(d, wo)
    good, bad = R.emulate_dztop(d, wo), R.emulate_dztop(d, wo, fault=fault)
    old = lambda x: np.abs(x - ref).max() < R.GRAD_TOL_OLD * np.abs(ref).max()
    assert old(good) and old(bad), fault
    lim = R.dztop_bound(dict(C=C))
    assert max(x[1] for x in R.dztop_slice_errors(good, ref, d, wo, lengths, valid)) <= lim
    assert [x for x in R.dztop_slice_errors(bad, ref, d, wo, lengths, valid) if not x[1] <= lim], fault


# ------------------------------------------------------------------------------------------------ 3: the table
def test_table_covers_the_variants_and_its_upt_arithmetic_holds():
    covered = {}
    for case in R.CASES:
        for v in case["covers"]:
            covered.setdefault(v, []).append(case)
    assert set(covered) == set(R.VARIANTS), set(covered) ^ set(R.VARIANTS)
    assert len(set(IDS)) == len(IDS)
    for case in R.CASES:
        L, H, B, T, C, U, plan = (case[k] for k in ("L", "H", "B", "T", "C", "U", "plan"))
        # the rules of csrc/lstm.hip the table's plans restate (the GPU test asserts the library's own answer against them)
        assert plan["nmt"] == (B + 15) // 16 and plan["kb"] == H // 128 and L * plan["nmt"] < 8
        assert plan["mv"] == int(case["precision"] == 0 and H == 512) and plan["w_pieces"] == (8 if T >= 64 else 0)
        assert C in (16, 32, 48, 64, 80) and 2 * U + 1 <= 384
        nteams = 2 * (8 - L * plan["nmt"]) * plan["nfw"]
        assert R.teams(case) == nteams and B <= 2 * nteams
        assert R.upt(case) == (2 if B > nteams else 1)
        if B > 3:
            assert case["labels"] == "standard"
    one = lambda v: covered[v][0]
    nt = lambda c: R.teams(c)
    assert R.upt(one("upt2-cap")) == 2 and one("upt2-cap")["B"] == 2 * nt(one("upt2-cap"))
    c = one("upt2-unreal")
    assert R.upt(c) == 2 and nt(c) < c["B"] < 2 * nt(c) - 1 and nt(c) == 40
    assert R.upt(one("upt1-edge")) == 1 and one("upt1-edge")["B"] == nt(one("upt1-edge"))
    assert R.upt(one("upt2-edge")) == 2 and one("upt2-edge")["B"] == nt(one("upt2-edge")) + 1
    assert one("ragged-tile")["B"] == 17
    assert {c["T"] for c in R.CASES} >= {t for _, t in CR.REQUIRED_T if t <= 17} | {1, 63, 64, 65}
    assert {c["C"] for c in R.CASES} == {16, 32, 48, 64, 80} and {c["H"] for c in R.CASES} == {128, 256, 384, 512}
    for extra, v in (("accumulate", "w8"), ("dropout", "dropout"), ("prefix", "prefix"), ("second", "second-batch")):
        assert any(extra in c["extras"] for c in covered[v]), extra
    assert one("prefix")["alloc_T"] > one("prefix")["T"] and one("second-batch")["first_T"] > one("second-batch")["T"]
    assert one("bf16x3")["precision"] == 1 and one("bf16")["precision"] == 2 and one("saturating")["regime"] == "saturating"
    # the four-wave case: every row has S >= 289 live states and its repeat where the name says
    c = one("waves4")
    lengths, dense = R.make_batch(c)
    for b in range(c["B"]):
        lab = dense[b][dense[b] != 0]
        assert 2 * len(lab) + 1 >= 289 and len(lab) == c["U"]
        u = ((97, 193, 289)[b % 3] - 1) // 2
        assert lab[u] == lab[u - 1]
    # the refusals: each breaks exactly one rule of ctc_head_nfw
    for what, L, H, B, T, C, U in R.REFUSALS:
        nmt = (B + 15) // 16
        broken = [C not in (16, 32, 48, 64, 80), 2 * U + 1 > 384, L * nmt >= 8, L * nmt < 8 and B > 4 * (8 - L * nmt) * 4]
        assert sum(broken) == 1 and L * nmt <= 8, what


# ------------------------------------------------------------------------------------------------ 4: the skip rule
@pytest.mark.parametrize("case", R.CASES, ids=IDS)
def test_no_slice_is_left_out_but_those_without_a_valid_frame_of_a_valid_row(case):
    inp, ref = R.reference_chain(case["name"])
    lengths, T, B, H, C = inp["lengths"], inp["T"], case["B"], case["H"], case["C"]
    valid = [v for v, _, _ in R.row_facts(inp["dense"], lengths, C)]
    for kind in S.OUTPUT_KINDS + S.GRAD_KINDS:
        errs = S.slice_errors(ref[kind], ref[kind], kind, lengths)
        label, _, frac = min(errs, key=lambda e: e[2])
        assert errs and frac >= R.FLOOR, "%s: slice %s has %.1e of the tensor's maximum" % (kind, label, frac)
    chunks = lambda n: (min(int(n), T) + 15) // 16
    lin = R.linear_slice_errors(ref["logits"], ref["logits"], lengths)
    assert len(lin) == sum(chunks(n) for n in lengths) * (C // 16)             # every (row, chunk, tile) with a valid frame
    assert min(x[2] for x in lin) >= R.FLOOR
    dz = R.dztop_slice_errors(ref["dztop"], ref["dztop"], ref["dlogits"], inp["wo"], lengths, valid)
    assert len(dz) == sum(chunks(n) for n, v in zip(lengths, valid) if v) * (H // 16)      # ... of a valid row
    label, _, frac = min(dz, key=lambda e: e[2])
    assert frac >= R.FLOOR, "dztop: slice %s has %.1e of the tensor's maximum" % (label, frac)
    # what is left out is exactly zero in the reference too (dlogits, dZ_top) or the bias alone (logits)
    zero = R.no_gradient_mask(T, lengths, valid)
    assert not ref["dlogits"][zero].any() and not ref["dztop"][zero].any()
    past = np.arange(T)[:, None] >= lengths[None, :]
    assert np.array_equal(ref["logits"][past], np.broadcast_to(inp["bo"].numpy(), ref["logits"].shape)[past])
    assert S.padding_is_zero(ref["ztop"], lengths) and S.padding_is_zero(ref["dz0"], lengths)
    assert np.isfinite(ref["loss"]).all() and all((ref["loss"][b] > 0) == valid[b] for b in range(B))


# ------------------------------------------------------------------------------------------------ 5: the labels
@pytest.mark.parametrize("case", R.CASES, ids=IDS)
def test_label_rows_fit_their_frames_but_for_the_deliberate_over_long_row(case):
    B, T, C, U = case["B"], case["T"], case["C"], case["U"]
    for TT in [T] + ([case["first_T"]] if case["first_T"] else []):
        lengths, dense = R.make_batch(case, TT)
        facts = R.row_facts(dense, lengths, C)
        assert dense.shape == (B, U) and dense.min() >= 0 and dense.max() <= C - 1 and lengths.max() == TT == lengths[0]
        special = {1, 3} if B > 3 else set()
        for b, (valid, required, need) in enumerate(facts):
            if b in special:
                assert not valid
                continue
            assert valid and required <= lengths[b] and need <= lengths[b], (b, required, need, lengths[b])
        if B > 3:
            assert lengths[1] == 0 and not dense[2].any() and facts[2][0] and lengths[3] > 0 and facts[3][1] > lengths[3]
