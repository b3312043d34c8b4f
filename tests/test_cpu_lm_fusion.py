"""First-pass fusion on the host, no GPU needed: the fused decoder of csrc/beam.cpp behind ops.ctc_beam_search_fused, driven by
stub language models whose rows are a hash of the WHOLE prefix (wrong parent / dest plumbing changes the answer) and that assert the
slot contract on every call; the lm_fusion configuration key and stt.build_rescorer; and the derived rounding bounds of the step
kernel against a float32 numpy evaluation and two wrong variants."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lm_fusion_ref as F  # noqa: E402
from rnn_speech_amd import lib, ops  # noqa: E402
from rnn_speech_amd.language_model import NbestRescorer  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _paths(ids, out_len):
    return [list(ids[b, :out_len[b]]) for b in range(ids.shape[0])]


# ---- 1. a constant language model changes nothing ------------------------------------------------------------------------
@pytest.mark.parametrize("width", (3, 8, 25))
@pytest.mark.parametrize("merge", (True, False))
def test_a_constant_model_gives_the_acoustic_nbest_bit_for_bit(width, merge):
    T, B, C, n_best = 24, 3, 5, 6
    rng = np.random.RandomState(width)
    lg = (rng.randn(T, B, C) * 1.5).astype(np.float32)
    lengths = np.array([T, T // 2, 0], np.int32)
    calls = []

    def zero_lm(parent, token, dest):
        calls.append((parent.copy(), token.copy(), dest.copy()))
        return np.zeros((len(parent), C), np.float32)

    got = ops.ctc_beam_search_fused(lg, lengths, zero_lm, n_best, width, merge, lm_weight=0.7, lm_length_bonus=0.0)
    want = ops.ctc_beam_search_nbest(lg, lengths, n_best, width, merge)
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and g.tobytes() == w.tobytes()
    one = ops.ctc_beam_search_fused(lg, lengths, zero_lm, 0, width, merge, lm_weight=0.7)
    assert one[0].tobytes() == want[0][:, 0].tobytes() and one[1].tobytes() == want[1][:, 0].tobytes()
    assert one[2].tobytes() == want[2][:, 0].tobytes()
    assert len(calls) <= 2 * (T + 1)                                          # two searches, at most T + 1 callbacks each
    roots = [c for c in calls if (c[0] == -1).any()]
    assert len(roots) == 2 and all(len(c[0]) == 1 and c[1][0] == C - 1 for c in roots)      # the root: once per search, alone
    n_slots = ops.ctc_beam_search_fused_slots(B, width)
    assert n_slots == B * 2 * width + 1 and all(c[2][0] == n_slots - 1 for c in roots)


def test_the_callbacks_come_once_per_frame_for_the_whole_batch_and_keep_the_slot_contract():
    T, B, C, width = 30, 3, 5, 6
    rng = np.random.RandomState(5)
    lg = rng.randn(T, B, C).astype(np.float32)
    stub = F.StubStepper(F.hash_lm(C, 9), C, ops.ctc_beam_search_fused_slots(B, width))
    ops.ctc_beam_search_fused(lg, [T, T // 2, 0], stub, 0, width, False, lm_weight=0.5, max_threads=2)
    assert stub.root_steps == 1 and stub.calls <= T + 1
    assert max(stub.rows) > width                                              # one call carried more than one utterance's entries
    assert max(max(s for s in stub.prefix_of), 0) < B * 2 * width + 1


# ---- 2. a beam wider than the number of prefixes finds the exact answer ---------------------------------------------------
@pytest.mark.parametrize("seed,T,C", [(0, 4, 3), (1, 5, 3), (2, 4, 4), (3, 5, 4), (4, 3, 4)])
def test_a_wide_beam_returns_the_brute_force_argmax(seed, T, C):
    rng = np.random.RandomState(40 + seed)
    lg = (rng.randn(T, C) * 1.5).astype(np.float32)
    lm = F.hash_lm(C, seed, sharp=2.0)
    w, bonus = 0.9, 0.4
    best, score, gap = F.brute_force_best(lg, C - 1, lm, w, bonus)
    assert gap > 1e-4, "choose another seed: the brute-force winner is not clear"
    width = sum((C - 1) ** n for n in range(T + 1)) + 1                        # more than there are prefixes
    stub = F.StubStepper(lm, C, ops.ctc_beam_search_fused_slots(1, width))
    ids, n, lp = ops.ctc_beam_search_fused(lg[:, None, :], [T], stub, 0, width, False, lm_weight=w, lm_length_bonus=bonus)
    assert list(ids[0, :n[0]]) == best
    assert abs(lp[0] - score) < 1e-4 * max(1.0, abs(score))
    assert stub.root_steps == 1 and stub.calls <= T + 1


# ---- 3. a narrow beam against the dictionary decoder ----------------------------------------------------------------------
@pytest.mark.parametrize("seed,T,C,width", F.NARROW_CASES)
def test_a_narrow_beam_equals_the_dictionary_decoder(seed, T, C, width):
    lg = F.narrow_case(seed, T, C)
    lm = F.hash_lm(C, seed)
    ranked, gap = F.fused_prefix_beam_search(lg, C - 1, width, lm, F.NARROW_LM_WEIGHT, F.NARROW_BONUS)
    assert gap > F.NARROW_GAP, "the case table must hold only seeds whose reference gap is clear (%g)" % gap
    stub = F.StubStepper(lm, C, ops.ctc_beam_search_fused_slots(1, width))
    ids, n, lp, found = ops.ctc_beam_search_fused(lg[:, None, :], [T], stub, width, width, False, F.NARROW_LM_WEIGHT, F.NARROW_BONUS)
    assert list(ids[0, 0, :n[0, 0]]) == ranked[0][0]
    assert abs(lp[0, 0] - ranked[0][1]) < 1e-3
    assert found[0] == len(ranked)
    assert stub.root_steps == 1 and stub.calls <= T + 1
    # prefixes did leave the beam and come back: more steps than distinct prefixes would need at most once each
    assert sum(stub.rows) >= len(set(stub.prefix_of.values()))


def test_a_returning_prefix_is_stepped_again_from_its_parent():
    """Some narrow case of the table steps one prefix twice (it left the beam and returned): the stub sees the same prefix at two
    calls, each time from a parent slot that holds its parent."""
    seen_twice = 0
    for seed, T, C, width in F.NARROW_CASES:
        lm = F.hash_lm(C, seed)
        steps = []

        class Recording(F.StubStepper):
            def __call__(self, parent, token, dest):
                out = F.StubStepper.__call__(self, parent, token, dest)
                steps.extend(self.prefix_of[int(d)] for d in dest)
                return out

        ops.ctc_beam_search_fused(F.narrow_case(seed, T, C)[:, None, :], [T], Recording(lm, C, 2 * width + 1), 0, width, False,
                                  F.NARROW_LM_WEIGHT, F.NARROW_BONUS)
        seen_twice += len(steps) - len(set(steps))
    assert seen_twice > 0


# ---- 4. fusion finds a path the acoustic n-best never held ----------------------------------------------------------------
def test_fusion_returns_a_path_outside_the_acoustic_nbest():
    T, C, width, n_best = 14, 5, 4, 4
    target = (0, 3, 1, 1, 2)
    rng = np.random.RandomState(21)
    lg = (rng.randn(T, 1, C) * 0.7).astype(np.float32)

    def lm(prefix):                       # sharp: the next token of `target`, then EOS; anything off the target wants EOS
        prefix = tuple(prefix)
        want = target[len(prefix)] if prefix == target[:len(prefix)] and len(prefix) < len(target) else C - 1
        z = np.full(C, -6.0)
        z[want] = 6.0
        return (z - np.log(np.exp(z).sum())).astype(np.float32)

    def scorer(id_lists):
        return [sum(float(lm(s[:k])[s[k]]) for k in range(len(s))) + float(lm(s)[C - 1]) for s in id_lists]

    nbest = ops.ctc_beam_search_nbest(lg, [T], n_best, width, False)
    acoustic = [list(nbest[0][0, k, :nbest[1][0, k]]) for k in range(nbest[3][0])]
    assert list(target) not in acoustic
    rescored = NbestRescorer(scorer, 1.0, lm_nbest=n_best)(lg, [T], width, False)
    stub = F.StubStepper(lm, C, ops.ctc_beam_search_fused_slots(1, width))
    ids, n, lp = ops.ctc_beam_search_fused(lg, [T], stub, 0, width, False, lm_weight=1.0)
    assert list(ids[0, :n[0]]) == list(target)
    assert _paths(*rescored)[0] != list(target) and _paths(*rescored)[0] in acoustic
    # and the fused score of the fused answer beats the same formula on the rescorer's pick
    lp64 = F.log_posteriors(lg[:, 0]).astype(np.float64)
    pick = _paths(*rescored)[0]
    assert lp[0] > F.ctc_log_prob(lp64, pick, C - 1) + scorer([pick])[0] + 1.0


# ---- 5. a callback status ends the call ------------------------------------------------------------------------------------
def test_a_callback_status_comes_back_after_exactly_that_call():
    T, B, C, width = 12, 2, 4, 3
    lg = np.random.RandomState(1).randn(T, B, C).astype(np.float32)
    calls = []

    def failing(parent, token, dest):
        calls.append(len(parent))
        return 7 if len(calls) == 3 else np.zeros((len(parent), C), np.float32)

    with pytest.raises(lib.AmdSpeechError, match=r"\(7\).*callback returned 7"):
        ops.ctc_beam_search_fused(lg, [T, T], failing, 0, width, True, lm_weight=0.5)
    assert len(calls) == 3

    def raising(parent, token, dest):
        calls.append(len(parent))
        raise KeyError("from the step")

    del calls[:]
    with pytest.raises(KeyError, match="from the step"):
        ops.ctc_beam_search_fused(lg, [T, T], raising, 0, width, True, lm_weight=0.5)
    assert len(calls) == 1
    with pytest.raises(lib.AmdSpeechError, match="bad arguments"):
        ops.ctc_beam_search_fused(lg, [T, T], failing, 0, 0, True)


# ---- 6. configuration and build_rescorer -----------------------------------------------------------------------------------
def test_lm_fusion_parses_defaults_to_rescore_and_is_not_structural(tmp_path):
    from rnn_speech_amd import hyperparams
    import stt
    src = open(os.path.join(ROOT, "config.ini")).read()
    assert hyperparams.read_config_file(os.path.join(ROOT, "config.ini"))["lm_fusion"] == "rescore"       # as shipped
    bare = tmp_path / "bare.ini"                                               # a file without the section
    bare.write_text(src.split("[lm_network_params]")[0] + "[logging]" + src.split("[logging]")[1])
    assert hyperparams.read_config_file(str(bare))["lm_fusion"] == "rescore"
    without = tmp_path / "without.ini"                                         # the section without the key
    without.write_text(src.replace("lm_fusion : rescore\n", ""))
    assert "\nlm_fusion :" not in without.read_text()
    assert hyperparams.read_config_file(str(without))["lm_fusion"] == "rescore"
    beam = tmp_path / "beam.ini"
    beam.write_text(src.replace("lm_fusion : rescore\n", "lm_fusion : Beam\n"))
    assert hyperparams.read_config_file(str(beam))["lm_fusion"] == "beam"
    assert "lm_fusion" not in hyperparams._STRUCTURAL
    both = tmp_path / "both.ini"
    both.write_text(src.replace("lm_fusion : rescore\n", "lm_fusion : both\n"))
    with pytest.raises(ValueError, match="lm_fusion"):
        hyperparams.read_config_file(str(both))
    # lm_weight 0: nothing is built, whatever lm_fusion says
    assert stt.build_rescorer({"lm_weight": 0, "lm_fusion": "beam"}) is None
    assert stt.build_rescorer({"lm_fusion": "beam"}) is None


# ---- 7. the derived bounds hold for a float32 evaluation and reject wrong steps -----------------------------------------
@pytest.fixture(scope="module")
def step_cases():
    return F.step_cases(ops.lm_step_plan)


def test_the_plan_reports_the_instantiations_and_the_table_straddles_them():
    ns = F.step_row_counts(ops.lm_step_plan)
    assert set(F.STEP_N_FIXED) <= set(ns)
    tiles = set()
    for n in ns:
        p = ops.lm_step_plan(n, 2, 256, 80)
        assert p["n_min"] <= n <= p["n_max"] and p["launches"] == 3 and p["kernel"] == "mfma16"
        assert p["row_tiles"] * p["row_tile"] >= n > (p["row_tiles"] - 1) * p["row_tile"]
        assert p["col_tiles"] * 16 == 256 and p["out_row_tiles"] * p["out_row_tile"] >= n
        assert p["lds_bytes"] <= 64 * 1024
        tiles.add(p["row_tile"])
        if p["n_max"] <= F.STEP_N_WALK_MAX:
            assert p["n_max"] in ns and p["n_max"] + 1 in ns
            assert ops.lm_step_plan(p["n_max"] + 1, 2, 256, 80)["row_tile"] != p["row_tile"]
        assert p["row_tile"] + 1 in ns
    assert len(tiles) >= 2
    for bad, word in (((1, 1, 24, 80), "multiple of 16"), ((1, 1, 16, 1), "at least 2"), ((0, 1, 16, 80), "positive"),
                      ((1, 9, 16, 80), "1 .. 8"), ((1, 0, 16, 80), "1 .. 8"), ((1, 1, 16, 257), "limit of 256"),
                      ((1, 1, 8192, 80), "limit of 4096")):
        with pytest.raises(lib.AmdSpeechError, match=word):
            ops.lm_step_plan(*bad)
    assert lib.load().amdspeech_lm_step_pool_bytes(201, 2, 256) == 201 * 2 * 256 * 4
    assert lib.load().amdspeech_lm_step_pool_bytes(201, 2, 250) == 0


def test_the_float32_step_meets_the_bounds_and_wrong_steps_miss_them_a_hundredfold(step_cases):
    worst = 0.0
    for case in step_cases:
        L, p = case["L"], case["params"]
        ref = F.lm_step_ref(p, L, case["h_par"], case["c_par"], case["token"])
        bounds = F.lm_step_bounds(p, L, case["h_par"], case["c_par"], case["token"])
        got = F.lm_step_f32(p, L, case["h_par"], case["c_par"], case["token"])
        for g, r, b in zip(got, ref, bounds):
            ratio = float((np.abs(g.astype(np.float64) - r) / b).max())
            worst = max(worst, ratio)
            assert ratio <= 1.0, (case["L"], case["H"], case["V"], case["N"], ratio)
        for variant in ("no_forget_bias", "neighbour_parent"):
            if variant == "neighbour_parent" and case["N"] < 2:
                continue
            bad = F.lm_step_f32(p, L, case["h_par"], case["c_par"], case["token"], variant=variant)
            miss = max(float((np.abs(g.astype(np.float64) - r) / b).max()) for g, r, b in zip(bad, ref, bounds))
            assert miss >= 100.0, (variant, case["L"], case["H"], case["V"], case["N"], miss)
    assert worst > 1e-3                      # the bounds are not vacuous: the float32 evaluation uses a visible part of them


def test_the_stepper_contract_check_names_what_is_wrong():
    from rnn_speech_amd.language_model import LmStepper
    chk = LmStepper.check_slots
    me = type("S", (), {"n_slots": 9})()
    i32 = lambda *v: np.array(v, np.int32)      # noqa: E731
    chk(me, i32(-1, 3, 3), i32(0, 1, 2))
    for parent, dest, word in ((i32(-1, 3), i32(4, 4), "same dest"), (i32(2, 3), i32(3, 5), "also a parent"),
                               (i32(-2, 3), i32(4, 5), "parent slot is outside"), (i32(-1, 3), i32(4, 9), "dest slot is outside")):
        with pytest.raises(ValueError, match=word):
            chk(me, parent, dest)
