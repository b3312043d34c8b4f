"""tests/ctc_align_ref.py tied down without a GPU, and the host side of the aligner's ABI: the float64 Viterbi against a brute-force
enumeration of every alignment (score and, under the tie rule, path), the emulated device arithmetic against the float64 path frame
by frame on seven cases of the matrix, tokens grouped into words, and amdspeech_ctc_align_workspace_bytes / amdspeech_ctc_align_plan."""
import ctypes
import itertools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ctc_align_ref as A  # noqa: E402
import ctc_ref as R  # noqa: E402

# the long / wide / peaky / large-logit cases on which the emulated device arithmetic is held to the float64 path frame by frame
EXACT_CASES = ("wave-full", "shift-long", "peaky-mid", "pair-long", "edge4-long", "large-edge4", "edge20-R")
ALPHABET, C = 4, 6                              # labels 1 .. 4, blank 5
TARGETS = [t for n in range(0, 4) for t in itertools.product(range(1, ALPHABET + 1), repeat=n)]


# ------------------------------------------------------------------------------------------------ reference == brute force
@pytest.mark.parametrize("kind", ["random", "equal"])
def test_reference_equals_brute_force_score_and_path(kind):
    """Every target of up to 3 labels over 4 symbols (repeats included), T = required time .. required + 3.  All-equal logits tie
    everywhere: there the path is decided by the tie rule alone."""
    rng = np.random.RandomState(5)
    checked = 0
    for tgt in TARGETS:
        ext, skip = A.extended(list(tgt), C)
        need = len(tgt) + sum(1 for u in range(1, len(tgt)) if tgt[u] == tgt[u - 1])
        for T in range(max(need, 1), max(need, 1) + 4):
            logits = (rng.randn(T, 1, C) * 2).astype(np.float32) if kind == "random" else np.zeros((T, 1, C), np.float32)
            lp = A.log_softmax64(logits)[:, 0]
            path, score, margins, fin_margin = A.viterbi(lp, ext, skip)
            bpath, bscore = A.brute(lp, ext, skip)
            assert path is not None and bpath is not None, (tgt, T)
            assert score == bscore, (tgt, T, score, bscore)
            assert (path == bpath).all(), (tgt, T, path, bpath)
            assert not A.validity(path, ext, skip, tgt, C), (tgt, T)
            assert abs(A.path_score(lp, ext, path) - score) <= 1e-12 * max(1.0, abs(score))
            if kind == "equal" and len(tgt) and T > need:
                assert margins[1:].min() == 0.0 or fin_margin == 0.0      # the ties this case is here for do occur
            checked += 1
    assert checked == len(TARGETS) * 4


def test_reference_says_no_alignment_where_repeats_need_more_frames():
    ext, skip = A.extended([2, 2, 3], C)
    lp = A.log_softmax64(np.zeros((3, 1, C), np.float32))[:, 0]      # three labels fit three frames by count, the repeat needs a fourth
    assert A.viterbi(lp, ext, skip)[0] is None and A.brute(lp, ext, skip)[0] is None


def test_tie_rule_smallest_step_and_last_state():
    """Spelled out on one row: all-equal logits, target (1, 2), 5 frames.  From the end: S-1 = 4 (the trailing blank) wins the last
    frame, then the walk stays as high as it can."""
    ext, skip = A.extended([1, 2], C)
    lp = A.log_softmax64(np.zeros((5, 1, C), np.float32))[:, 0]
    path = A.viterbi(lp, ext, skip)[0]
    assert path.tolist() == [1, 3, 4, 4, 4]


# ------------------------------------------------------------------------------------------------ emulation == float64, frame by frame
@pytest.mark.parametrize("name", EXACT_CASES)
def test_emulated_path_equals_float64_path_in_every_frame(name):
    c = R.by_name(name)
    logits, dense, lengths, info = R.build(c)
    ref = A.align(logits, dense, lengths)
    emu = A.align(logits, dense, lengths, emulate=True)
    for b, (r, e, i) in enumerate(zip(ref, emu, info)):
        assert (r is None) == (not i["valid"])
        if r is None:
            continue
        assert (r["path"] is None) == i["inf"]
        if r["path"] is None:
            continue
        assert (r["path"] == e["path"]).all(), "%s row %d: %d frames differ" % (name, b, int((r["path"] != e["path"]).sum()))
        assert abs(e["score"] - r["score"]) <= 3e-5, (name, b, e["score"] - r["score"])
        smallest = min(float(r["margins"].min()), r["fin_margin"])
        print("%s row %d: Tb %d S %d  emulated score error %.2e  smallest margin %.2e  bound %.2e"
              % (name, b, r["Tb"], len(r["ext"]), abs(e["score"] - r["score"]), smallest, A.bound(r, e)))
        # (the smallest margins -- 3.9e-5 on shift-long row 1 -- are above the emulation's own score error everywhere, which is why the
        # two paths agree; they are NOT all above the row's bound, whose floor Tb * 2^-23 * max|log p| is 1.8e-3 at Tb = 1001: the GPU
        # test's exception for a stretch that starts at such a decision can apply there, and it prints how often it did)
        assert smallest > 2 * abs(e["score"] - r["score"])


def test_every_case_aligns_the_rows_the_loss_keeps():
    """Over the whole matrix: ignored rows are ignored, impossible rows have no path, every other path is valid."""
    for c in R.CASES:
        if c["T"] > 600 and c["name"] not in EXACT_CASES:
            continue                                   # (the long cases cost seconds each; the GPU test runs them all)
        logits, dense, lengths, info = R.build(c)
        for b, (r, i) in enumerate(zip(A.align(logits, dense, lengths), info)):
            assert (r is None) == (not i["valid"]), (c["name"], b)
            if r is None:
                continue
            assert (r["path"] is None) == i["inf"], (c["name"], b)
            if r["path"] is not None:
                assert (r["ext"] == i["ext"]).all()
                assert not A.validity(r["path"], r["ext"], r["skip"], r["tgt"], c["C"]), (c["name"], b)
                assert abs(A.path_score(r["lp"], r["ext"], r["path"]) - r["score"]) <= 1e-9 * max(1.0, abs(r["score"]))


def test_ladder_restated_covers_every_case_width():
    for c in R.CASES:
        kernel, rmax, threads = A.expected_plan(c["U"])
        assert 2 * c["U"] + 1 <= rmax * threads


# ------------------------------------------------------------------------------------------------ the ABI, host side
@pytest.fixture(scope="module")
def lib():
    import rnn_speech_amd.lib as L
    return L.load()


def test_align_workspace_bytes_is_the_documented_sum_and_monotone_in_T(lib):
    for T, B, C_, U in ((20, 3, 80, 8), (1001, 32, 80, 161), (1001, 32, 80, 255), (1300, 32, 80, 1100), (3510, 10, 80, 600), (7, 1, 3, 2559),
                        (45, 2, 4096, 63)):
        n = lib.amdspeech_ctc_align_workspace_bytes(T, B, C_, U)
        assert n > 0 and n == A.workspace_bytes(T, B, C_, U), (T, B, C_, U, n)
        assert lib.amdspeech_ctc_align_workspace_bytes(T + 1, B, C_, U) > n
    for bad in ((0, 1, 80, 8), (5, 0, 80, 8), (5, 1, 1, 8), (5, 1, 80, 0)):
        assert lib.amdspeech_ctc_align_workspace_bytes(*bad) == 0


def test_align_plan_answers_at_the_ladder_edges_and_refuses_2560(lib):
    import rnn_speech_amd.lib as L
    from rnn_speech_amd import ops
    for U in (1, 63, 64, 255, 256, 511, 512, 1023, 1024, 1535, 1536, 2047, 2048, 2559):
        kernel, rmax, threads = A.expected_plan(U)
        assert ops.ctc_align_plan(1001, 4, 80, U) == {"kernel": kernel, "threads": threads, "rmax": rmax, "smax": 2 * U + 1}, U
    assert ops.ctc_align_plan(10, 1, 80, 63)["kernel"] == "wave" and ops.ctc_align_plan(10, 1, 80, 64)["kernel"] == "edge"
    info = L.CtcPlanInfo()
    for call in (lib.amdspeech_ctc_align_plan, lib.amdspeech_ctc_plan):      # the same limits, the same messages
        assert call(10, 1, 80, 2560, ctypes.byref(info)) != 0
        assert b"exceeds the supported 2559" in lib.amdspeech_last_error()
        assert call(10, 1, 4097, 8, ctypes.byref(info)) != 0
        assert b"too large" in lib.amdspeech_last_error()
        assert call(10, 1, 1, 8, ctypes.byref(info)) != 0
        assert b"bad shape" in lib.amdspeech_last_error()
    with pytest.raises(L.AmdSpeechError):
        ops.ctc_align_plan(10, 1, 80, 2560)


def test_loss_workspace_bytes_unchanged(lib):
    """The aligner has its own workspace: the loss's query answers what its layout (csrc/ctc_core.h: ctc_layout) always answered."""
    up = lambda n: (n + 255) // 256 * 256
    for T, B, C_, U in ((20, 3, 80, 8), (1001, 32, 80, 161), (300, 2, 80, 600), (64, 2, 29, 70)):
        smax = 2 * U + 1
        want = up(T * B * C_ * 4) + 2 * up(B * T * smax * 4) + up(B * smax * 4) + 3 * up(B * 4)
        assert lib.amdspeech_ctc_workspace_bytes(T, B, C_, U) == want


# ------------------------------------------------------------------------------------------------ tokens -> words
def test_group_words_inverts_the_codec():
    from rnn_speech_amd import labels as Lb
    cm = Lb.ENGLISH_CHAR_MAP
    ids = Lb.get_str_labels(cm, Lb.clean_label("It'll do, well-being"), add_eos=True)
    tokens = [(t, 3 * i, 3 * i + 1, 0.9 - 0.01 * i) for i, t in enumerate(ids)]
    words = Lb.group_words(cm, tokens)
    assert " ".join(w[0] for w in words) == Lb.get_labels_str(cm, ids) == "it'll do well being"
    assert words[0][1] == 0 and all(a[2] < b[1] for a, b in zip(words, words[1:]))
    n0 = len(Lb.get_str_labels(cm, "it'll", add_eos=False))
    assert words[0][2] == 3 * (n0 - 1) + 1 and abs(words[0][3] - (0.9 - 0.01 * (n0 - 1))) < 1e-12      # last token's frame; the minimum
