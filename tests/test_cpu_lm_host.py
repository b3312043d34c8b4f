"""Host side of the language model, no GPU needed: the n-best list of the beam decoder against the single-path call and against
a brute-force enumeration, LanguageModel.build_dataset on the reference's stub sentences, the new configuration section, and the
n-best rescoring rule with a stub scorer."""
import itertools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

from rnn_speech_amd import labels, ops  # noqa: E402
from rnn_speech_amd.language_model import LanguageModel, NbestRescorer, rescore_nbest, sentence_rows  # noqa: E402

CHAR_MAP = labels.ENGLISH_CHAR_MAP


def _logits(T, B, C, seed, peaked=False):
    rng = np.random.RandomState(seed)
    x = rng.randn(T, B, C).astype(np.float32)
    if peaked:
        x *= 3.0
    return x


@pytest.mark.parametrize("exhaustive", ("0", "1"))
@pytest.mark.parametrize("merge", (True, False))
def test_nbest_entry_zero_is_the_single_path_answer(monkeypatch, exhaustive, merge):
    monkeypatch.setenv("AMDSPEECH_BEAM_EXHAUSTIVE", exhaustive)
    T, B, C, width, n_best = 23, 4, 9, 12, 7
    logits = _logits(T, B, C, 3, peaked=True)
    logits[:, 1] = logits[:, 0]                     # ties between rows cost nothing; row 2 is short, row 3 empty
    lengths = np.array([T, T, 5, 0], np.int32)
    ids1, len1, lp1 = ops.ctc_beam_search(logits, lengths, width, merge)
    ids, out_len, lp, found = ops.ctc_beam_search_nbest(logits, lengths, n_best, width, merge)
    assert ids.shape == (B, n_best, T) and out_len.shape == lp.shape == (B, n_best)
    assert np.array_equal(ids[:, 0], ids1) and np.array_equal(out_len[:, 0], len1)
    assert np.array_equal(lp[:, 0].view(np.uint32), lp1.view(np.uint32))                      # bit for bit
    assert list(found[:3]) == [n_best] * 3 and found[3] == 1                                  # an empty utterance: the empty prefix alone
    for b in range(B):
        n = found[b]
        assert np.all(np.diff(lp[b, :n]) <= 0)                                                # scores never increase
        assert np.all(lp[b, n:] == -np.inf) and np.all(out_len[b, n:] == 0) and np.all(ids[b, n:] == C)
        for k in range(n):
            assert np.all(ids[b, k, out_len[b, k]:] == C) and np.all(ids[b, k, :out_len[b, k]] < C - 1)
        if not merge:
            paths = {tuple(ids[b, k, :out_len[b, k]]) for k in range(n)}
            assert len(paths) == n                                                            # unmerged paths are pairwise distinct


def _brute_force(logits_tc):
    """log P(prefix) over ALL alignments of one utterance, float64: {prefix: log probability}."""
    T, C = logits_tc.shape
    x = logits_tc.astype(np.float64)
    lp = x - np.log(np.exp(x - x.max(1, keepdims=True)).sum(1, keepdims=True)) - x.max(1, keepdims=True)
    blank = C - 1
    acc = {}
    for path in itertools.product(range(C), repeat=T):
        prefix = tuple(k for k, _ in itertools.groupby(path) if k != blank)
        p = sum(lp[t, c] for t, c in enumerate(path))
        acc[prefix] = np.logaddexp(acc[prefix], p) if prefix in acc else p
    return acc


def test_nbest_equals_brute_force_enumeration_and_fills_unused_slots():
    T, B, C, width = 4, 2, 3, 64
    logits = _logits(T, B, C, 11)
    lengths = np.array([T, T], np.int32)
    for b in range(B):
        truth = _brute_force(logits[:, b])
        n_prefixes = len(truth)
        assert n_prefixes < width
        n_best = n_prefixes + 3                                      # more than the beam can hold: the rest is filled as specified
        ids, out_len, lp, found = ops.ctc_beam_search_nbest(logits, lengths, n_best, width, merge_repeated=False)
        assert found[b] == n_prefixes
        got = {tuple(ids[b, k, :out_len[b, k]]): float(lp[b, k]) for k in range(found[b])}
        assert set(got) == set(truth)
        for prefix, logp in truth.items():
            assert abs(got[prefix] - logp) <= 1e-5 * max(1.0, abs(logp)), (prefix, got[prefix], logp)
        order = sorted(truth, key=lambda p: -truth[p])
        gaps = np.diff([truth[p] for p in order])
        assert np.all(np.abs(gaps) > 1e-4)                           # (no near-tie: the float32 order must be the float64 order)
        assert [tuple(ids[b, k, :out_len[b, k]]) for k in range(found[b])] == order
        assert np.all(lp[b, found[b]:] == -np.inf) and np.all(out_len[b, found[b]:] == 0) and np.all(ids[b, found[b]:] == C)
    with pytest.raises(Exception, match="n_best"):
        ops.ctc_beam_search_nbest(logits, lengths, 0, width)


def test_build_dataset_rows_of_the_reference_stub_sentences():
    sentences = ["the brown lazy fox", "the red quick fox", "the yellow quick fox", "the green lazy fox"]
    C = len(CHAR_MAP)
    batches = LanguageModel.build_dataset(sentences, 3, 20, CHAR_MAP)
    assert [(t.shape, l.shape, n) for t, l, n in batches] == [((3, 22), (3,), 3), ((3, 22), (3,), 1)]
    rows = np.concatenate([t for t, _, _ in batches])
    lens = np.concatenate([l for _, l, _ in batches])
    assert rows.dtype == np.int32 and lens.dtype == np.int32
    for b, text in enumerate(sentences):
        ids = labels.get_str_labels(CHAR_MAP, text, add_eos=False)
        assert lens[b] == len(ids) + 1
        assert list(rows[b, :len(ids) + 2]) == [C - 1] + ids + [C - 1]          # [start, tokens, EOS]
        assert np.all(rows[b, len(ids) + 2:] == C - 1)
        assert labels.get_labels_str(CHAR_MAP, rows[b, 1:len(ids) + 1]) == text
    assert list(lens[4:]) == [0, 0]                                               # the last batch is padded with empty rows
    # "the brown lazy fox": T h e B r o w n L a z y F o x, no multi-character token
    assert [CHAR_MAP[i] for i in rows[0, 1:lens[0]]] == list("TheBrownLazyFox")
    # double letters are one token: the row is one shorter than the text has letters
    tok, lens2 = sentence_rows([labels.get_str_labels(CHAR_MAP, "the green lazy fox", add_eos=False)], C)
    assert lens2[0] == len("TheGreenLazyFox") - 1 + 1 and CHAR_MAP[tok[0, 6]] == "ee"      # [start, T, h, e, G, r, ee, ...]


def test_build_dataset_skips_sentences_that_are_too_long(caplog):
    long_one = "a" * 30 + " b"
    with caplog.at_level("WARNING"):
        batches = LanguageModel.build_dataset(["the red quick fox", long_one, "fox"], 2, 20, CHAR_MAP)
    assert sum(n for _, _, n in batches) == 2 and "1 of 3 sentences" in caplog.text
    assert LanguageModel.build_dataset([long_one], 2, 20, CHAR_MAP) == []


def test_the_language_model_section_parses_with_defaults(tmp_path):
    from rnn_speech_amd import hyperparams
    src = open(os.path.join(ROOT, "config.ini")).read()
    d = hyperparams.read_config_file(os.path.join(ROOT, "config.ini"))
    assert (d["lm_num_layers"], d["lm_hidden_size"], d["lm_dropout"], d["lm_batch_size"]) == (2, 256, 0.9, 64)
    assert (d["lm_learning_rate"], d["lm_lr_decay_factor"], d["lm_grad_clip"]) == (0.001, 0.5, 5)
    assert (d["lm_text_files"], d["lm_weight"], d["lm_nbest"], d["lm_length_bonus"]) == ([], 0, 16, 0)
    assert (d["num_layers"], d["hidden_size"], d["batch_size"]) == (3, 512, 32)               # the acoustic section is its own
    bare = tmp_path / "bare.ini"                    # a config.ini written before the section existed
    bare.write_text(src.split("[lm_network_params]")[0] + "[logging]" + src.split("[logging]")[1])
    b = hyperparams.read_config_file(str(bare))
    assert {k: v for k, v in b.items() if k.startswith("lm_")} == {k: v for k, v in d.items() if k.startswith("lm_")}
    assert not any(k.startswith("lm_") for k in hyperparams._STRUCTURAL)                      # none is structural
    changed = tmp_path / "changed.ini"
    changed.write_text(src.replace("lm_weight : 0", "lm_weight : 0.7").replace("lm_text_files :", "lm_text_files : a.txt, b.txt")
                       .replace("lm_nbest : 16", "lm_nbest : 4"))
    c = hyperparams.read_config_file(str(changed))
    assert (c["lm_weight"], c["lm_text_files"], c["lm_nbest"]) == (0.7, ["a.txt", "b.txt"], 4)
    for bad in ("lm_weight : -1", "lm_nbest : 0", "lm_weight : much"):
        key = bad.split(" : ")[0]
        wrong = tmp_path / "wrong.ini"
        wrong.write_text("\n".join(bad if l.startswith(key + " :") else l for l in src.splitlines()))
        with pytest.raises(ValueError, match=key):
            hyperparams.read_config_file(str(wrong))


def test_the_modes_keep_their_order_and_train_language_is_one():
    import stt
    names = [name for name, _, _ in stt._MODES]
    assert names == ["train_acoustic", "train_language", "file", "record", "evaluate", "generate_text", "align", "feature_stats"]
    assert "not supported" not in dict((n, t) for n, _, t in stt._MODES)["train_language"]
    assert "not supported" in dict((n, t) for n, _, t in stt._MODES)["generate_text"]


def test_train_language_refuses_a_data_parallel_job(monkeypatch, tmp_path):
    import stt
    src = open(os.path.join(ROOT, "config.ini")).read().replace("checkpoint_dir : data/checkpoints/", "checkpoint_dir : %s" % tmp_path)
    cfg = tmp_path / "config.ini"
    cfg.write_text(src)
    monkeypatch.setenv("WORLD_SIZE", "2")
    monkeypatch.setattr(sys, "argv", ["stt.py", "--train_language", "--config", str(cfg)])
    with pytest.raises(SystemExit) as ex:
        stt.main()
    assert "one process" in str(ex.value.code)


def test_a_missing_checkpoint_is_an_error_that_names_the_directory(tmp_path):
    class _NoEngine(LanguageModel):
        def _create(self):
            self.rnn_created = True

    model = _NoEngine(1, 16, 2, 20, 20, 80)
    model.create_forward_rnn()
    assert model.restore(None, str(tmp_path)) is False
    with pytest.raises(RuntimeError) as ex:
        model.restore(None, str(tmp_path), must_exist=True)
    assert os.path.join(str(tmp_path), "language") in str(ex.value) and "languagemodel.npz" in str(ex.value)
    import stt
    assert stt.build_rescorer({"lm_weight": 0}) is None and stt.build_rescorer({}) is None


def _nbest_fixture():
    """Two utterances, three slots each, T 4, C 6: utterance 0 holds a duplicate (slots 0 and 2 spell the same ids after merging)."""
    C, T = 6, 4
    ids = np.full((2, 3, T), C, np.int32)
    out_len = np.zeros((2, 3), np.int32)
    rows = {(0, 0): [1, 2], (0, 1): [1, 3], (0, 2): [1, 2], (1, 0): [4], (1, 1): [4, 4, 0]}
    for (b, k), r in rows.items():
        ids[b, k, :len(r)] = r
        out_len[b, k] = len(r)
    log_prob = np.array([[-1.0, -1.5, -1.6], [-2.0, -2.25, -np.inf]], np.float32)
    return ids, out_len, log_prob, np.array([3, 2], np.int32)


def test_rescoring_picks_the_combined_argmax_and_deduplicates():
    ids, out_len, log_prob, found = _nbest_fixture()
    seen = []

    def scorer(cands):
        seen.append([tuple(c) for c in cands])
        table = {(1, 2): -3.0, (1, 3): -1.0, (4,): -1.0, (4, 4, 0): -0.25}
        return [table[tuple(c)] for c in cands]

    got_ids, got_len, got_lp = rescore_nbest(ids, out_len, log_prob, found, scorer, lm_weight=0.5)
    # utterance 0: -1 + 0.5 * -3 = -2.5 against -1.5 + 0.5 * -1 = -2.0 -> slot 1;  utterance 1: -2.5 against -2.375 -> slot 1
    assert list(got_ids[0]) == [1, 3, 6, 6] and got_len[0] == 2 and got_lp[0] == np.float32(-1.5)
    assert list(got_ids[1]) == [4, 4, 0, 6] and got_len[1] == 3
    assert seen == [[(1, 2), (1, 3), (4,), (4, 4, 0)]]               # ONE call for the mini-batch, the duplicate dropped, best score kept
    # a length bonus moves utterance 1 back: -2 - 0.5 - 1 against -2.25 - 0.125 - 3
    got_ids, got_len, _ = rescore_nbest(ids, out_len, log_prob, found, scorer, lm_weight=0.5, lm_length_bonus=-1.0)
    assert got_len[1] == 1 and list(got_ids[1]) == [4, 6, 6, 6]


def test_rescoring_at_weight_zero_returns_entry_zero_untouched():
    ids, out_len, log_prob, found = _nbest_fixture()

    def scorer(cands):
        raise AssertionError("the scorer must not be called at lm_weight 0")

    got_ids, got_len, got_lp = rescore_nbest(ids, out_len, log_prob, found, scorer, lm_weight=0)
    assert np.array_equal(got_ids, ids[:, 0]) and np.array_equal(got_len, out_len[:, 0]) and np.array_equal(got_lp, log_prob[:, 0])


def test_the_rescorer_decodes_scores_and_returns_a_path_per_utterance():
    T, B, C = 12, 3, 6
    logits = _logits(T, B, C, 5, peaked=True)
    lengths = np.array([T, 7, T], np.int32)
    best_ids, best_len, _ = ops.ctc_beam_search(logits, lengths, 8, True)
    nb = ops.ctc_beam_search_nbest(logits, lengths, 4, 8, True)
    # a scorer that loves the SECOND distinct hypothesis of every utterance
    second = []
    for b in range(B):
        seqs = []
        for k in range(nb[3][b]):
            s = tuple(nb[0][b, k, :nb[1][b, k]])
            if s not in seqs:
                seqs.append(s)
        second.append(seqs[1])
    sharp = NbestRescorer(lambda cands: [0.0 if tuple(c) in second else -100.0 for c in cands], lm_weight=1.0, lm_nbest=4)
    ids, out_len = sharp(logits, lengths, 8, True)
    for b in range(B):
        assert tuple(ids[b, :out_len[b]]) == second[b] != tuple(best_ids[b, :best_len[b]])
    flat = NbestRescorer(lambda cands: [0.0] * len(cands), lm_weight=1.0, lm_nbest=4)      # an indifferent model changes nothing
    ids, out_len = flat(logits, lengths, 8, True)
    assert np.array_equal(ids, best_ids) and np.array_equal(out_len, best_len)
