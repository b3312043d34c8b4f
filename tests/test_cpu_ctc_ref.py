"""tests/ctc_ref.py tied down without a GPU: the float64 oracle against torch.nn.functional.ctc_loss autograd in float64, the closure
of the case matrix over the recursion kernels' thread layouts (and that the suite's six older cases do NOT close it), the proof that
the slice metric and the row-sum invariant catch three planted faults, and that no case leaves a row or a frame out."""
import importlib.util
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ctc_ref as R  # noqa: E402

RUNS = [(c["name"], m) for c, m in R.runs()]


# ------------------------------------------------------------------------------------------------ the oracle
@pytest.mark.parametrize("name", [c["name"] for c in R.CASES])
def test_oracle_matches_torch_ctc_loss_in_float64(name):
    """Every valid row with a finite loss (torch has no ignore_longer_outputs_than_inputs and no TF-style inf handling)."""
    ev = R.evaluated(name, next(iter(R.by_name(name)["plan"])))
    c, info = ev["case"], ev["info"]
    keep = [b for b, i in enumerate(info) if i["valid"] and not i["inf"]]
    assert keep
    lg = torch.tensor(ev["logits"][:, keep].astype(np.float64), requires_grad=True)
    lens = torch.tensor([i["Tb"] for i in (info[b] for b in keep)])
    tl = torch.tensor([info[b]["n"] for b in keep])
    tgt = torch.tensor(np.concatenate([info[b]["ext"][1::2] for b in keep] + [np.zeros(0, np.int64)]))
    loss = torch.nn.functional.ctc_loss(torch.log_softmax(lg, 2), tgt, lens, tl, blank=c["C"] - 1, reduction="none")
    loss.sum().backward()
    ref_loss, ref_d = ev["ref_loss"][keep], ev["ref_d"][:, keep]
    assert np.abs(loss.detach().numpy() - ref_loss).max() <= 1e-9 * max(1.0, np.abs(ref_loss).max())
    assert np.abs(lg.grad.numpy() - ref_d).max() <= 1e-9


def test_reference_is_float64_finite_and_positive_except_where_a_case_says_inf():
    for c in R.CASES:
        ev = R.evaluated(c["name"], next(iter(c["plan"])))
        assert ev["ref_d"].dtype == np.float64 and ev["ref_loss"].dtype == np.float64
        assert np.isfinite(ev["ref_d"]).all()
        for b, (i, r) in enumerate(zip(ev["info"], c["rows"])):
            if i["inf"]:
                assert "inf" in c["tags"] and r["kind"] == "impossible" and np.isposinf(ev["ref_loss"][b])
            elif i["valid"]:
                assert np.isfinite(ev["ref_loss"][b]) and ev["ref_loss"][b] > 0, (c["name"], b)
            else:
                assert ev["ref_loss"][b] == 0 and not ev["ref_d"][:, b].any()
        assert ("inf" in c["tags"]) == any(i["inf"] for i in ev["info"])


# ------------------------------------------------------------------------------------------------ nothing is left out
def test_frame_blocks_partition_the_valid_frames():
    for Tb in list(range(0, 70)) + [127, 128, 129, 1001, 2563]:
        blocks = R.frame_blocks(Tb)
        assert [a for a, _ in blocks] == [0][:len(blocks) and 1] + [b for _, b in blocks[:-1]]
        assert (blocks[-1][1] if blocks else 0) == Tb and all(a < b for a, b in blocks)
        if Tb > 32:
            assert blocks[0] == (0, 16) and blocks[-1] == (Tb - 16, Tb)


@pytest.mark.parametrize("name,mode", RUNS)
def test_every_row_and_frame_of_a_case_is_in_a_slice_with_a_bound(name, mode):
    ev = R.evaluated(name, mode)
    c = ev["case"]
    keys = set(ev["bounds"])
    for b in range(c["B"]):
        assert ("loss", b) in keys
        Tb = min(int(ev["lengths"][b]), c["T"])
        covered = sorted((k[2], k[3]) for k in keys if k[0] == "d" and k[1] == b)
        assert sum(t1 - t0 for t0, t1 in covered) == Tb and (not covered or (covered[0][0] == 0 and covered[-1][1] == Tb))
    for k, bound in ev["bounds"].items():
        cap = R.LOSS_CAP if k[0] == "loss" else R.D_CAP
        assert 0 < bound <= cap
        # the emulated arithmetic itself holds the suite's tolerance on every slice (else the bound would be the cap and the
        # arithmetic, not the test, would be what is wrong -- the float32 state was: see the test below)
        assert ev["emu_err"][k] <= cap, (k, ev["emu_err"][k])
    assert ev["emu_rowsum"] <= R.D_CAP
    assert (ev["plan"][0], ev["plan"][1]) == tuple(c["plan"][mode])


def test_float32_state_misses_the_tolerance_where_long_meets_wide_and_float64_holds_it():
    """The finding that moved the LDS-exchange kernels to a float64 state: emulated with the state in float32, dlogits is further
    than the suite's 2e-3 from float64 at the long-and-wide cases; with the state in float64 what remains is the float32 storage of
    alpha / beta (their ulp at |alpha| ~ 5000 is 5e-4) and stays under it."""
    for name in ("edge20-long", "edge4-long", "pair-long"):
        new = R.evaluated(name, "default")
        old = R.evaluated(name, "default", fam=new["fam"] + "-f32")
        worst = lambda ev: max(e for k, e in ev["emu_err"].items() if k[0] == "d")
        print("%s: float32 state %.2e, float64 state %.2e" % (name, worst(old), worst(new)))
        assert worst(old) > R.D_CAP > 2 * worst(new)


# ------------------------------------------------------------------------------------------------ closure of the matrix
def test_the_matrix_reaches_every_kernel_R_wave_and_repeat_position():
    rows = R.matrix_rows()
    assert not R.closure_missing(rows), sorted(R.closure_missing(rows), key=str)
    plans = {(p[0], p[1]) for p, _, _, _ in rows}
    assert plans == {("wave", 2), ("shift", 2), ("pair", 2), ("edge", 2), ("edge", 4), ("edge", 8), ("edge", 20)}
    # full width (S == smax or smax - 2) with a shorter row beside it and T not a multiple of 16, per kernel and mode
    for mode in R.MODES:
        for kr in plans:
            ok = False
            for c in R.CASES:
                if c["plan"].get(mode) != kr or c["T"] % 16 == 0:
                    continue
                S = [2 * r["n"] + 1 for r in c["rows"] if r["kind"] == "valid"]
                ok |= bool(S) and max(S) >= 2 * c["U"] - 1 and min(S) < max(S)
            if any(c["plan"].get(mode) == kr for c in R.CASES):
                assert ok, (mode, kr)
    for mode, kernels in (("default", {"wave", "shift", "pair", "edge"}), ("shift0", {"wave", "pair"}), ("pair0", {"wave", "edge"})):
        assert {c["plan"][mode][0] for c in R.CASES if mode in c["plan"]} == kernels
    # the dispatch edges, the alphabets, the T edges, mixed rows with B in {1, 5}, the long-and-wide shapes
    assert {63, 64, 191, 192, 255, 256, 511, 512, 1023, 1024, 2559} <= {c["U"] for c in R.CASES}
    assert {3, 29, 64, 65, 80, 1000, 4096} <= {c["C"] for c in R.CASES}
    for kernel in ("wave", "shift", "pair", "edge"):
        assert {1, 2, 7, 8, 9} <= {c["T"] for c in R.CASES if c["plan"]["default"][0] == kernel}
        assert any("inf" in c["tags"] for c in R.CASES if c["plan"]["default"][0] == kernel)
    for kernel in ("shift", "pair", "edge"):
        kinds = [{r["kind"] for r in c["rows"]} for c in R.CASES if c["plan"]["default"][0] == kernel and c["B"] == 5]
        assert any({"valid", "len0", "empty", "toolong"} <= k for k in kinds)
        assert any(c["B"] == 1 for c in R.CASES if c["plan"]["default"][0] == kernel)
    shapes = {(c["T"], c["U"]) for c in R.CASES if 2 <= c["B"] <= 3 and max(r["n"] for r in c["rows"]) == c["U"]}
    assert {(1300, 1100), (1001, 511), (1001, 255), (1001, 191)} <= shapes
    assert {"random", "peaky", "large"} == {c["logits"] for c in R.CASES}


def test_the_older_cases_do_not_close_the_matrix():
    """The finding this matrix answers: make_ctc_case draws the target length from lengths // 2, so the suite's six cases leave the
    upper waves, every R above 2, the kernels for 385 .. 1024 states and the wave boundaries of the DPP kernel unreached."""
    miss = R.closure_missing(R.old_rows())
    assert {("R", "edge4", 1), ("R", "edge8", 2), ("R", "edge20", 3), ("R", "edge20", 20), ("wave", "edge8", 3), ("wave", "shift", 3), ("wave", "pair", 3),
            ("S=", "shift", 383), ("S=", "pair", 511), ("long", "shift"), ("rep-wave", "shift", 1)} <= miss
    assert len(miss) > 60


@pytest.mark.parametrize("drop,lost", [("edge20-R", ("R", "edge20", 20)), ("edge8-full", ("R", "edge8", 8)), ("shift-T17", ("T=", "shift", 17)),
                                       ("edge-R3-repeats", ("rep", "edge8", 0))])
def test_closure_fails_when_a_wide_case_leaves_the_matrix(drop, lost):
    rows = R.matrix_rows([c for c in R.CASES if c["name"] != drop])
    assert lost in R.closure_missing(rows)


# ------------------------------------------------------------------------------------------------ the emulation and its teeth
def test_wave_layout_of_the_dpp_kernel_equals_the_plain_recursion_bit_for_bit():
    """The overlapping wave windows with their 16-frame refresh compute what the plain recursion computes (that is the kernel's claim);
    the emulation of the layout is what the late-refresh fault is planted in."""
    ev = R.evaluated("shift-waves", "default")
    with np.errstate(all="ignore"):
        loss, d = R.emulate(ev["logits"], ev["dense"], ev["lengths"], ("shift", 2, 256), fam="shift-waves")
    assert np.array_equal(loss, ev["emu_loss"]) and np.array_equal(d, ev["emu_d"])


def _old_case(T, B, C, U):
    spec = importlib.util.spec_from_file_location("old_gpu_kernels", os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_gpu_kernels.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.make_ctc_case(T, B, C, U, seed=T + B)


@pytest.mark.parametrize("fault,name,old", [("skip_first", "edge-R3-repeats", (300, 2, 80, 600)), ("late_halo", "exact-U150", (64, 2, 29, 70)),
                                            ("final_one", "pair-full-255", (257, 3, 80, 161))])
def test_planted_faults_fail_the_slice_metric_on_a_full_width_case(fault, name, old):
    """(A late halo refresh shows only where the paths that carry the posterior run at full speed, T == required time + 1: a path one
    step behind crosses the bottom of a wave's window just after a refresh and reaches the first owned lane 17 frames later.  With
    frames to spare, alpha is wrong only at states whose lag the rest of the utterance cannot make up -- beta is -inf there -- or by less
    than a float32 resolves, which is why the kernel may recompute its halo for 16 frames at all.)"""
    ev = R.evaluated(name, "default")
    with np.errstate(all="ignore"):
        loss, d = R.emulate(ev["logits"], ev["dense"], ev["lengths"], ev["plan"], fault=fault)
    fails, worst = R.judge(ev, loss, d)
    assert fails and worst > 4, (fault, worst)
    good, worst_good = R.judge(ev, ev["emu_loss"], ev["emu_d"])
    assert not good and worst_good < 1.0          # (the emulation itself sits at 1 / FACTOR of its bound, or nearer where the cap binds)
    # the same fault on the older, narrow case of that kernel against the older whole-tensor check
    logits, dense, lengths = _old_case(*old)
    with np.errstate(all="ignore"):
        loss, d = R.emulate(logits, dense, lengths, R.expected_plan(old[3]), fault=fault)
    ref_loss, ref_d = R.reference(logits, dense, lengths)
    passes_old = np.abs(d - ref_d).max() < 2e-3 and np.abs(loss - ref_loss).max() / np.abs(ref_loss).max() < 2e-5
    print("%s on the old case %r: whole-tensor max %.2e -> %s" % (fault, old, np.abs(d - ref_d).max(), "passes" if passes_old else "fails"))
    if fault == "late_halo":
        assert passes_old          # no live state above wave 0 there: the fault is invisible to the older suite


# ------------------------------------------------------------------------------------------------ the plan query (host code only)
def test_ctc_plan_at_the_dispatch_edges_and_its_refusals():
    from rnn_speech_amd import lib, ops
    for U in (1, 12, 63, 64, 191, 192, 255, 256, 511, 512, 1023, 1024, 2559):
        plan = ops.ctc_plan(7, 3, 80, U)
        kernel, rmax, threads = R.expected_plan(U)
        assert plan == dict(kernel=kernel, rmax=rmax, threads=threads, smax=2 * U + 1), (U, plan)
    for c in R.CASES:
        plan = ops.ctc_plan(c["T"], c["B"], c["C"], c["U"])
        assert (plan["kernel"], plan["rmax"]) == c["plan"]["default"], c["name"]
    for bad in ((7, 3, 80, 2560), (7, 3, 4097, 10), (7, 3, 1, 10), (0, 3, 80, 10), (7, 0, 80, 10), (7, 3, 80, 0)):
        with pytest.raises(lib.AmdSpeechError):
            ops.ctc_plan(*bad)
    assert ops.ctc_plan(7, 3, 4096, 10)["kernel"] == "wave"


@pytest.mark.parametrize("mode", ["shift0", "pair0"])
def test_ctc_plan_honours_the_fallback_switches(mode):
    """The switches are read once per process: a child asks."""
    import subprocess
    code = ("import sys; sys.path.insert(0, %r); from rnn_speech_amd import ops\n"
            "print([(U, ops.ctc_plan(9, 2, 80, U)['kernel'], ops.ctc_plan(9, 2, 80, U)['rmax']) for U in (63, 64, 191, 192, 255, 256, 2559)])"
            % os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **R.MODES[mode]), capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    assert eval(out.stdout.strip().splitlines()[-1]) == [(U,) + R.expected_plan(U, mode)[:2] for U in (63, 64, 191, 192, 255, 256, 2559)]
