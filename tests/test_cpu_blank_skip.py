"""Blank-frame skipping without a GPU: the float64 reference against hand-written answers, the case table (every frame decided), the
float32 emulation of the kernels inside the derived bound, planted faults that each miss a named case, the decode_blank_skip key, the
prototypes, and decoder invariance through the host decoders of csrc/beam.cpp on the numpy compaction -- with the negative control
that shows why the first frame of a run is kept."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import blank_skip_ref as R  # noqa: E402
import lm_fusion_ref as F  # noqa: E402
from rnn_speech_amd import hyperparams, lib, ops  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def table():
    return R.cases(ops.ctc_blank_skip_plan)


def _case(table, name):
    hits = [c for c in table if c["name"] == name]
    assert len(hits) == 1, name
    return hits[0]


# ---- 1. the reference ------------------------------------------------------------------------------------------------------
def _frames(pattern, C=3):
    """'b' a blank frame (blank 20 above), 'x' a label frame; one utterance."""
    x = np.zeros((len(pattern), 1, C), np.float32)
    for t, ch in enumerate(pattern):
        x[t, 0, C - 1 if ch == "b" else 0] = 20.0
    return x


@pytest.mark.parametrize("pattern,n,kept", [
    ("xxxx", 4, [0, 1, 2, 3]),                  # nothing skippable: the input itself
    ("bbbb", 4, [0]),                           # one frame survives
    ("xbxbx", 5, [0, 1, 2, 3, 4]),              # runs of one lose nothing
    ("bbxx", 4, [0, 2, 3]),                     # a run that starts at t = 0
    ("xxbbb", 5, [0, 1, 2]),                    # a run that ends at n - 1
    ("xbbxbbbx", 8, [0, 1, 3, 4, 7]),
    ("xbbbbb", 3, [0, 1]),                      # blank-looking frames at t >= n are not kept
    ("xxbb", 9, [0, 1, 2]),                     # a length beyond T is T
    ("xbbx", -2, []),
    ("xbbx", 0, []),
    ("bbbb", 1, [0]),
])
def test_the_reference_gives_the_hand_written_answers(pattern, n, kept):
    x = _frames(pattern)
    T = len(pattern)
    ref = R.blank_skip_ref(x, [n], 0.9)
    assert ref["out_lengths"].tolist() == [len(kept)]
    assert ref["src_frame"][0].tolist() == kept + [-1] * (T - len(kept))
    assert ref["out_logits"][:len(kept), 0].tobytes() == x[kept, 0].tobytes()
    assert not ref["out_logits"][len(kept):].any()
    assert not ref["blank_logp"][max(min(n, T), 0):].any()


def test_the_reference_keeps_a_nan_frame_and_takes_equality_at_theta_one():
    x = _frames("xbbbx")
    x[2, 0, 1] = np.nan                                                      # inside the run: kept, and it ends the run before it
    ref = R.blank_skip_ref(x, [5], 0.9)
    assert np.isnan(ref["blank_logp"][2, 0]) and ref["src_frame"][0].tolist() == [0, 1, 2, 3, 4]
    y = _frames("xbbx")
    y[1:3, 0, 2] = 90.0                                                      # dominance 90: lpb exactly 0 = log(1)
    ref = R.blank_skip_ref(y, [4], 1.0)
    assert ref["blank_logp"][1, 0] == 0.0 and ref["src_frame"][0].tolist() == [0, 1, 3, -1]
    ref = R.blank_skip_ref(_frames("xbbx"), [4], 1.0)                        # dominance 20: lpb = -4e-9 < 0, nothing skippable
    assert ref["out_lengths"].tolist() == [4]


def test_none_skippable_returns_the_input_bit_for_bit(table):
    for name in ("T513_B3_C5_none", "T9_B3_C80_none"):
        c = _case(table, name)
        ref = R.blank_skip_ref(c["logits"], c["lengths"], c["theta"])
        n = R.clip_lengths(c["lengths"], c["T"])
        for b in range(c["B"]):
            assert ref["out_lengths"][b] == n[b]
            assert ref["src_frame"][b, :n[b]].tolist() == list(range(n[b]))
            assert ref["out_logits"][:n[b], b].tobytes() == c["logits"][:n[b], b].tobytes()
    c = _case(table, "T513_B3_C5_all")
    assert R.blank_skip_ref(c["logits"], c["lengths"], c["theta"])["out_lengths"].tolist() == [1, 1, 1]


# ---- 2. the table ----------------------------------------------------------------------------------------------------------
def test_the_table_covers_what_it_must_and_every_frame_is_decided(table):
    plan = ops.ctc_blank_skip_plan
    ch = plan(3, 3, 5)["t_chunk"]
    Cs, Ts, Bs = {c["C"] for c in table}, {c["T"] for c in table}, {c["B"] for c in table}
    assert {2, 5, 80, 81} <= Cs and {1, 2, 3, ch - 1, ch, ch + 1, 2 * ch + 1} <= Ts and {1, 3, 33} <= Bs
    c = 2
    while c <= R.C_MAX:                                                      # both sides of every boundary the plan reports
        p = plan(3, 3, c)
        assert p["c_min"] == c and c in Cs and p["c_max"] in Cs
        assert plan(3, 3, p["c_max"])["words_per_lane"] == p["words_per_lane"] and plan(3, 3, p["c_max"])["kernel"] == p["kernel"]
        c = p["c_max"] + 1
    assert c == R.C_MAX + 1
    assert {plan(c["T"], c["B"], c["C"])["kernel"] for c in table} == {"wave", "block"}
    assert {plan(c["T"], c["B"], c["C"])["vec"] for c in table} == {1, 4}
    assert {c["pattern"] for c in table} == set(R.PATTERNS)
    lens = np.concatenate([np.asarray(c["lengths"]) - c["T"] for c in table if c["B"] >= 5])
    assert {0, 5}.issubset(lens.tolist()) and any((np.asarray(c["lengths"]) < 0).any() for c in table)
    for c in table:
        bad = R.undecided(c["logits"], c["lengths"], c["theta"])
        assert not bad.any(), "%s: %d undecided frames" % (c["name"], bad.sum())
    assert any(c["theta"] == 1.0 for c in table) and any(np.isnan(c["logits"]).any() for c in table)
    assert sum(c["logits"].size for c in table) < 2_000_000                  # (the GPU tests stay quick)


def test_the_plan_names_its_limits():
    plan = ops.ctc_blank_skip_plan
    p = plan(1001, 32, 80)
    assert p["kernel"] == "wave" and p["vec"] == 4 and p["launches"] == 3 and p["scan_grid"] == 32 and p["rows_grid"] == 1001 * 32 // 4
    assert p["chunks"] == -(-1001 // p["t_chunk"]) and p["gather_grid"] == -(-1001 * 32 * 20 // p["gather_threads"])
    assert plan(2, 2, 4097 - 1)["kernel"] == "block" and plan(2, 2, 1024)["kernel"] == "wave" and plan(2, 2, 1025)["kernel"] == "block"
    load = lib.load()
    assert load.amdspeech_ctc_blank_skip_workspace_bytes(1001, 32, 80) >= 1001 * 32
    for T, B, C, word in ((0, 1, 5, "at least 1"), (1, 0, 5, "at least 1"), (3, 3, 1, "below 2"), (3, 3, 4097, "4096"),
                          (1 << 15, 1 << 10, 64, "2^31")):
        with pytest.raises(lib.AmdSpeechError, match=re.escape(word)):
            plan(T, B, C)
        assert load.amdspeech_ctc_blank_skip_workspace_bytes(T, B, C) == 0
    assert load.amdspeech_ctc_blank_skip_plan(3, 3, 4097, None) != 0


# ---- 3. the float32 emulation and the planted faults --------------------------------------------------------------------------
def test_the_float32_emulation_stays_inside_the_bound_and_decides_as_float64(table):
    worst = 0.0
    for c in table:
        plan = ops.ctc_blank_skip_plan(c["T"], c["B"], c["C"])
        ref = R.blank_skip_ref(c["logits"], c["lengths"], c["theta"])
        got = R.blank_skip_f32(c["logits"], c["lengths"], c["theta"], plan)
        with np.errstate(invalid="ignore"):
            M = np.nanmax(np.abs(c["logits"].astype(np.float64)), axis=2)
        bound = R.lpb_bound(c["C"], M)
        err = np.abs(got["blank_logp"].astype(np.float64) - ref["blank_logp"])
        assert np.array_equal(np.isnan(err), np.isnan(ref["blank_logp"])), c["name"]
        ok = np.isnan(err) | (err <= bound)
        assert ok.all(), "%s: |lpb_f32 - lpb_f64| = %g above the bound %g" % (c["name"], np.nanmax(err / bound), 1.0)
        worst = max(worst, float(np.nanmax(err / bound)))
        assert R.same_outputs(got, ref), c["name"]
    print("largest |lpb_f32 - lpb_f64| / bound over the table: %.3g" % worst)
    assert worst > 0.0                                                       # (the emulation is not the reference in disguise)


@pytest.mark.parametrize("fault,name", [
    ("keep_last", "T9_B3_C80_run_at_start"),
    ("seam_reset", "T513_B3_C5_seam"),
    ("count_past_length", "T9_B3_C80_past_length"),
    ("gt_not_ge", "T5_B3_C4096_theta_one"),
    ("tail_not_zeroed", "T9_B3_C80_all"),
])
def test_a_planted_fault_misses_its_named_case(table, fault, name):
    c = _case(table, name)
    plan = ops.ctc_blank_skip_plan(c["T"], c["B"], c["C"])
    ref = R.blank_skip_ref(c["logits"], c["lengths"], c["theta"])
    assert R.same_outputs(R.blank_skip_f32(c["logits"], c["lengths"], c["theta"], plan), ref)
    assert not R.same_outputs(R.blank_skip_f32(c["logits"], c["lengths"], c["theta"], plan, fault=fault), ref)
    if fault == "gt_not_ge":                                                 # the constructed equality: lpb is exactly 0 = log(1)
        lpb = R.blank_logp_f32(c["logits"], c["lengths"], plan["words_per_lane"], plan["rows_threads"], plan["vec"])
        assert (lpb[ref["skip"]] == 0.0).all() and ref["skip"].any()


# ---- 4. configuration and prototypes -------------------------------------------------------------------------------------------
def test_decode_blank_skip_parses_defaults_to_off_and_names_its_range(tmp_path):
    src = open(os.path.join(ROOT, "config.ini")).read()
    assert "\ndecode_blank_skip : 0\n" in src
    hp = hyperparams.HyperParameterHandler(os.path.join(ROOT, "config.ini")).get_hyper_params()
    assert hp["decode_blank_skip"] == 0.0
    old = tmp_path / "old.ini"                                               # a file from before the key: off
    old.write_text("\n".join(l for l in src.splitlines() if not l.startswith("decode_blank_skip")) + "\n")
    assert hyperparams.HyperParameterHandler(str(old)).get_hyper_params()["decode_blank_skip"] == 0.0
    for text, want in (("0.95", 0.95), ("1", 1.0), ("1.0", 1.0), ("0.50001", 0.50001)):
        assert hyperparams.read_decode_keys(lambda k, d: text)["decode_blank_skip"] == want
    for text in ("0.5", "0.3", "1.01", "-0.9", "nan", "inf", "yes"):
        with pytest.raises(ValueError, match="above 0.5 and at most 1"):
            hyperparams.read_decode_keys(lambda k, d: text)
    assert "decode_blank_skip" not in hyperparams._STRUCTURAL
    on = tmp_path / "on.ini"
    on.write_text(src.replace("decode_blank_skip : 0\n", "decode_blank_skip : 0.98\n"))
    assert hyperparams.HyperParameterHandler(str(on)).get_hyper_params()["decode_blank_skip"] == 0.98


def test_the_prototypes_hold_the_three_symbols():
    for name in ("amdspeech_ctc_blank_skip_workspace_bytes", "amdspeech_ctc_blank_skip_plan", "amdspeech_ctc_blank_skip"):
        assert name in lib.PROTOTYPES and hasattr(lib.load(), name)
        assert re.search(r"\b%s\(" % name, open(os.path.join(ROOT, "include", "amdspeech.h")).read())
    assert [n for n, _ in lib.BlankSkipPlanInfo._fields_] == re.search(
        r"typedef struct amdspeech_ctc_blank_skip_plan_info \{\s*int ([^;]+);", open(os.path.join(ROOT, "include", "amdspeech.h")).read()
    ).group(1).replace("\n", " ").replace(" ", "").split(",")


# ---- 5. the decoders see the same thing ---------------------------------------------------------------------------------------
T_DEC, B_DEC, C_DEC, WIDTH = 60, 3, 6, 16


@pytest.fixture(scope="module", params=(0.5, 0.75, 0.9))
def peaky(request):
    x, lengths, in_run = R.peaky_posteriors(T_DEC, B_DEC, C_DEC, request.param, seed=int(100 * request.param))
    ref = R.blank_skip_ref(x, lengths, 0.95)
    assert not R.undecided(x, lengths, 0.95).any()
    live = np.arange(T_DEC)[:, None] < lengths[None, :]
    assert np.array_equal(ref["skip"], in_run & live)                        # exactly the run frames are skippable ...
    lpb32 = R.blank_logp_f32(x, lengths, 4, 64, 1)
    assert (lpb32[ref["skip"]] == 0.0).all()                                 # ... and their lpb is exactly 0.0 in float32
    m = int(ref["out_lengths"].max())
    assert 0 < m < T_DEC
    return x, lengths, ref["out_logits"][:m].copy(), ref["out_lengths"]


@pytest.mark.parametrize("merge", (True, False))
def test_the_beam_decoders_return_the_same_paths_on_the_compacted_input(peaky, merge):
    x, lengths, small, new_len = peaky
    full = ops.ctc_beam_search(x, lengths, WIDTH, merge)
    comp = ops.ctc_beam_search(small, new_len, WIDTH, merge)
    Tc = small.shape[0]
    assert np.array_equal(full[1], comp[1]) and (full[1] <= Tc).all()
    for b in range(B_DEC):
        assert full[0][b, :full[1][b]].tolist() == comp[0][b, :comp[1][b]].tolist()
    assert np.abs(full[2] - comp[2]).max() < 1e-4
    n_best = 4
    full = ops.ctc_beam_search_nbest(x, lengths, n_best, WIDTH, merge)
    comp = ops.ctc_beam_search_nbest(small, new_len, n_best, WIDTH, merge)
    assert np.array_equal(full[3], comp[3]) and np.array_equal(full[1], comp[1]) and (full[3] == n_best).all()
    for b in range(B_DEC):
        for k in range(n_best):
            assert full[0][b, k, :full[1][b, k]].tolist() == comp[0][b, k, :comp[1][b, k]].tolist()
    assert np.abs(full[2] - comp[2]).max() < 1e-4


def test_the_fused_decoder_returns_the_same_paths_in_fewer_step_calls(peaky):
    x, lengths, small, new_len = peaky
    out, calls = [], []
    for lg, ln in ((x, lengths), (small, new_len)):
        stub = F.StubStepper(F.hash_lm(C_DEC, 9), C_DEC, ops.ctc_beam_search_fused_slots(B_DEC, WIDTH))
        out.append(ops.ctc_beam_search_fused(lg, ln, stub, 0, WIDTH, True, lm_weight=0.5))
        calls.append(stub.calls)
        assert stub.root_steps == 1
    full, comp = out
    assert np.array_equal(full[1], comp[1])
    for b in range(B_DEC):
        assert full[0][b, :full[1][b]].tolist() == comp[0][b, :comp[1][b]].tolist()
    assert np.abs(full[2] - comp[2]).max() < 1e-4
    # the decoder's ceiling is one call per frame it is handed and the root's: it falls from T + 1 to max(new_lengths) + 1.  (A
    # frame from which no new prefix enters a beam makes no call -- csrc/beam.cpp -- so on peaky input the full search already
    # stays below its ceiling; the exact count is pinned by the next test, where the beam never fills.)
    assert calls[1] <= int(new_len.max()) + 1 < T_DEC + 1 and calls[1] <= calls[0] <= int(lengths.max()) + 1


def test_the_fused_decoder_makes_one_step_call_per_kept_frame_and_the_root():
    """With a beam wider than the number of prefixes the kept frames can spell, every frame brings a new prefix into the beam, so
    the fused search calls `step` exactly once per frame it is handed: max(new_lengths) + 1 calls instead of T + 1."""
    C, width = 3, 100
    x = np.clip(np.random.RandomState(4).randn(8, 1, C), -1.0, 1.0).astype(np.float32)
    for t, c in enumerate((0, 2, 2, 2, 1, 2, 2, 0)):                         # a _ _ _ b _ _ a
        x[t, 0, c] = 85.0 if c == 2 else 6.0
    ref = R.blank_skip_ref(x, [8], 0.95)
    assert ref["src_frame"][0].tolist() == [0, 1, 4, 5, 7, -1, -1, -1] and sum(2 ** n for n in range(6)) < width
    out, calls = [], []
    for lg, ln in ((x, [8]), (ref["out_logits"][:5], ref["out_lengths"])):
        stub = F.StubStepper(F.hash_lm(C, 2), C, ops.ctc_beam_search_fused_slots(1, width))
        out.append(ops.ctc_beam_search_fused(lg, ln, stub, 0, width, True, lm_weight=0.5))
        calls.append(stub.calls)
    assert calls[1] == int(ref["out_lengths"].max()) + 1 == 6 and calls[1] < calls[0] <= 8 + 1
    assert out[0][0][0, :out[0][1][0]].tolist() == out[1][0][0, :out[1][1][0]].tolist() == [0, 1, 0]
    assert abs(out[0][2][0] - out[1][2][0]) < 1e-4


def test_dropping_whole_runs_merges_a_repeated_label():
    """The negative control: "a _ a" with the blank run dropped completely decodes to "a"; with its first frame kept, to "a a".
    (merge_repeated off: on, TensorFlow's rule collapses equal neighbours of the OUTPUT, and "a a" reads "a" either way.)"""
    C = 3
    x = np.full((6, 1, C), -5.0, np.float32)
    for t, c in enumerate((0, 2, 2, 2, 0, 2)):                               # a _ _ _ a _
        x[t, 0, c] = 85.0 if c == 2 else 5.0
    ref = R.blank_skip_ref(x, [6], 0.95)
    assert ref["src_frame"][0].tolist() == [0, 1, 4, 5, -1, -1]
    want = ops.ctc_beam_search(x, [6], WIDTH, False)
    assert want[0][0, :want[1][0]].tolist() == [0, 0]
    kept = ops.ctc_beam_search(ref["out_logits"][:4], ref["out_lengths"], WIDTH, False)
    assert kept[0][0, :kept[1][0]].tolist() == [0, 0]
    whole = x[[0, 4]]                                                        # every skippable frame dropped, no first-of-run kept
    lost = ops.ctc_beam_search(whole, [2], WIDTH, False)
    assert lost[0][0, :lost[1][0]].tolist() == [0]
