"""The language model on the GPU (rnn_speech_amd.language_model) against the float64 oracle -- oracle.model on one-hot input plus
lm_ref's cross-entropy --, its scoring and training, its checkpoint, and n-best rescoring through stt.py."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lm_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

STUB_TRAIN = ["the brown lazy fox", "the red quick fox"]      # the reference's stub training sentences


def rel_err(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-30))


def _batch(V, lens, width, seed):
    """Rows [V-1, y.., V-1] with lens[b] - 1 random tokens each, padded with V-1 to width + 1."""
    from rnn_speech_amd.language_model import sentence_rows
    rng = np.random.RandomState(seed)
    return sentence_rows([list(rng.randint(0, V - 1, size=n - 1)) for n in lens], V, width=width)


def _engine(L, H, V, B, T, seed=7):
    from rnn_speech_amd.language_model import LmEngine
    eng = LmEngine(L, H, V, B, T, seed=seed)
    rng = np.random.RandomState(1)
    p = eng.to_numpy()
    for k in p:                               # non-zero biases exercise the bias paths
        if p[k].ndim == 1:
            p[k] = (rng.randn(*p[k].shape) * 0.1).astype(np.float32)
    eng.load_numpy(p)
    return eng, {k: v.astype(np.float64) for k, v in p.items()}


# L, H, the LSTM path the shape takes: the whole-sequence dataflow kernels, and the launch-per-diagonal kernels
@pytest.mark.parametrize("L,H,path", [(2, 128, "flow"), (1, 16, "diag")])
@pytest.mark.parametrize("keep", [(1.0, 1.0), (0.8, 0.5)], ids=["dropout-off", "dropout-on"])
def test_lm_step_matches_the_oracle(L, H, path, keep):
    from test_gpu_dropout_oracle import engine_masks
    V, B, T = 80, 3, 12
    eng, p64 = _engine(L, H, V, B, T)
    tok, lens = _batch(V, [12, 7, 1], T, seed=H)
    d_tok, d_len = torch.as_tensor(tok).cuda(), torch.as_tensor(lens).cuda()
    eng.zero_grads()
    eng.mini_batch(d_tok, d_len, keep[0], keep[1], seed=4242, max_len=int(lens.max()))
    torch.cuda.synchronize()
    eng.check()
    got = eng.kernel_path()
    assert (got["lstm_fwd"], got["lstm_bwd"], got["run_length"]) == (path, path, 12), got
    masks = (None, None) if keep == (1.0, 1.0) else engine_masks(eng._ws, L)      # (the descriptor still holds this step's keep / seed)
    loss_ref, logits_ref, g_ref = R.lm_oracle_loss_and_grads(p64, tok, lens, L, in_masks=masks[0], out_masks=masks[1])
    np.testing.assert_allclose(eng.loss.cpu().numpy(), loss_ref, rtol=1e-3, atol=1e-5)
    logits = eng.logits.cpu().numpy()
    assert np.abs(logits - logits_ref).max() < 1e-3 * np.abs(logits_ref).max()
    g = eng.to_numpy(eng.grads)
    for k in g_ref:
        assert rel_err(g[k], g_ref[k]) < 2e-3, (k, rel_err(g[k], g_ref[k]))
    # the rows of input_w whose token occurs nowhere in the batch got no gradient at all
    absent = np.setdiff1d(np.arange(V), np.concatenate([tok[b, :lens[b]] for b in range(B)]))
    assert len(absent) > 0 and np.all(g["input_w"][absent] == 0)
    if keep != (1.0, 1.0):                   # and the masks matter
        assert rel_err(R.lm_oracle_loss_and_grads(p64, tok, lens, L)[1], logits_ref) > 1e-2
    # scale: the gradient of the same step at scale 1/7 is a seventh
    eng.zero_grads()
    eng.mini_batch(d_tok, d_len, keep[0], keep[1], seed=4242, max_len=int(lens.max()), scale=1.0 / 7.0)
    g7 = eng.to_numpy(eng.grads)
    for k in g_ref:
        assert rel_err(7.0 * g7[k], g[k]) < 1e-4, k


def test_score_does_not_depend_on_the_batch_and_equals_the_oracle():
    from rnn_speech_amd.language_model import LanguageModel
    V = 80
    model = LanguageModel(2, 128, 3, 20, 20, V, seed=11)
    model.create_forward_rnn()
    rng = np.random.RandomState(4)
    seqs = [list(rng.randint(0, V - 1, size=n)) for n in (5, 19, 0, 11, 2, 20, 7)]
    together = model.score(seqs)                                   # three batches: 3 + 3 + 1
    alone = np.array([model.score([s])[0] for s in seqs])
    np.testing.assert_allclose(alone, together, rtol=1e-5)
    mixed = model.score([seqs[0], seqs[5], seqs[1]])               # with longer rows
    np.testing.assert_allclose(mixed, together[[0, 5, 1]], rtol=1e-5)
    assert model.score([list(range(21))])[0] == -np.inf            # longer than max_target_seq_length: no score
    p64 = {k: v.astype(np.float64) for k, v in model.engine.to_numpy().items()}
    from rnn_speech_amd.language_model import sentence_rows
    tok, lens = sentence_rows(seqs, V)
    loss_ref, _, _ = R.lm_oracle_loss_and_grads(p64, tok, lens, 2)
    np.testing.assert_allclose(together, -loss_ref, rtol=1e-3, atol=1e-5)
    # per-token scores add up to the row's
    d_tok, d_len = model._device_batch(*sentence_rows(seqs[:3], V, width=21))
    logp, per_token = model.engine.score(d_tok, d_len, per_token=True)
    assert per_token.shape == (21, 3) and np.all(per_token <= 0)
    np.testing.assert_allclose(per_token.sum(axis=0), logp, rtol=1e-6)
    np.testing.assert_allclose(logp, together[:3], rtol=1e-5)


def test_thirty_steps_on_the_stub_sentences_lower_the_loss():
    from rnn_speech_amd import labels
    from rnn_speech_amd.language_model import LanguageModel
    char_map = labels.ENGLISH_CHAR_MAP
    model = LanguageModel(2, 128, 2, 20, 20, len(char_map), seed=3)
    model.create_training_rnn(0.9, 0.9, 5.0, 1e-2, 0.5)
    dataset = LanguageModel.build_dataset(STUB_TRAIN, 2, 20, char_map)
    first, _ = model.evaluate_dataset(dataset)
    assert abs(first - np.log(80)) < 0.5                            # a fresh model is near the uniform distribution
    losses = []
    for _ in range(30):
        model.add_dataset_input(dataset)
        loss, err, step, exhausted = model.run_train_step(None, 1)
        losses.append(loss)
    assert step == 30 and 0.0 <= err <= 1.0
    last, last_err = model.evaluate_dataset(dataset)
    print("mean token NLL: first %.4f, last %.4f (ln 80 = %.4f), token error %.3f" % (first, last, np.log(80), last_err))
    assert last < first and last < np.log(80) and losses[-1] < losses[0]
    assert model.recovered_steps == 0
    # the trained model prefers a training sentence to its reversal
    ids = labels.get_str_labels(char_map, STUB_TRAIN[0], add_eos=False)
    s = model.score([ids, ids[::-1]])
    assert s[0] > s[1]


def test_save_then_restore_reproduces_the_scores_bit_for_bit(tmp_path):
    from rnn_speech_amd import labels
    from rnn_speech_amd.language_model import LanguageModel
    char_map = labels.ENGLISH_CHAR_MAP
    model = LanguageModel(1, 32, 2, 20, 20, len(char_map), seed=5)
    model.create_training_rnn(1.0, 1.0, 5.0, 1e-2, 0.5)
    dataset = LanguageModel.build_dataset(STUB_TRAIN, 2, 20, char_map)
    for _ in range(3):
        model.add_dataset_input(dataset)
        model.run_train_step(None, 1)
    seqs = [labels.get_str_labels(char_map, t, add_eos=False) for t in STUB_TRAIN + ["fox"]]
    before = model.score(seqs)
    model.save(None, str(tmp_path))
    assert os.path.exists(os.path.join(str(tmp_path), "language", "languagemodel.npz"))
    z = np.load(LanguageModel.checkpoint_path(str(tmp_path)))
    assert {"Input_Layer/input_w", "rnn/multi_rnn_cell/cell_0/basic_lstm_cell/kernel", "Output_layer/output_b", "global_step",
            "learning_rate", "adam/step", "adam/m/Input_Layer/input_w"} <= set(z.files)
    assert z["Input_Layer/input_w"].shape == (80, 32) and int(z["global_step"]) == 3 and int(z["adam/step"]) == 3
    other = LanguageModel(1, 32, 2, 20, 20, len(char_map), seed=99)
    other.create_training_rnn(1.0, 1.0, 5.0, 1e-2, 0.5)
    assert not np.array_equal(other.score(seqs), before)
    assert other.restore(None, str(tmp_path)) is True
    assert np.array_equal(other.score(seqs).view(np.uint64), before.view(np.uint64))
    assert other.global_step.value == 3 and other.engine.adam_step == 3
    # ... and training goes on from the same optimiser state
    for flat in ("params", "adam_m", "adam_v"):
        assert np.array_equal(getattr(model.engine, flat).cpu().numpy(), getattr(other.engine, flat).cpu().numpy()), flat
    assert np.float32(other.get_learning_rate()) == np.float32(model.get_learning_rate())


CONFIG = """
[acoustic_network_params]
num_layers : 1
hidden_size : 32
dropout_input_keep_prob : 0.8
dropout_output_keep_prob : 0.5
batch_size : 2
mini_batch_size : 2
learning_rate : 0.001
lr_decay_factor : 0.33
grad_clip : 1
signal_processing : mfcc
language : english
rnn_state_reset_ratio : 0.25

[general]
use_config_file_if_checkpoint_exists : True
steps_per_checkpoint : 2
steps_per_evaluation : 2
checkpoint_dir : %(dir)s/ckpt

[training]
training_dataset_dirs : %(dir)s/train.tsv
test_dataset_dirs : %(dir)s/test.tsv
max_input_seq_length : 60
max_target_seq_length : 20
batch_normalization : False
dataset_size_ordering : True
%(lm)s
[logging]
log_level : WARNING
"""

LM_SECTION = """
[lm_network_params]
num_layers : 1
hidden_size : 32
dropout : 0.9
batch_size : 4
learning_rate : 0.01
lr_decay_factor : 0.5
grad_clip : 5
lm_text_files : %(text)s
lm_weight : %(weight)s
lm_nbest : 8
lm_length_bonus : 0
"""


def test_stt_rescoring_with_a_sharp_language_model(tmp_path, monkeypatch, capsys):
    from test_gpu_stt import write_wav
    import stt
    import util.hyperparams as hyperparams
    from models.SpeechRecognizer import SpeechRecognizer
    from rnn_speech_amd import labels
    from rnn_speech_amd.language_model import LanguageModel
    d = str(tmp_path)
    wav = os.path.join(d, "u0.wav")
    write_wav(wav, 0)

    def config(name, lm):
        path = os.path.join(d, name)
        with open(path, "w") as fh:
            fh.write(CONFIG % {"dir": d, "lm": lm})
        return path

    def run_file(cfg):
        monkeypatch.setattr(sys, "argv", ["stt.py", "--file", wav, "--config", cfg])
        stt.main()
        return capsys.readouterr().out

    parent_cfg = config("parent.ini", "")                            # a configuration written before the section existed
    off_cfg = config("off.ini", LM_SECTION % {"text": "", "weight": "0"})
    on_cfg = config("on.ini", LM_SECTION % {"text": "", "weight": "1.0"})
    # a tiny acoustic checkpoint, saved as the command line restores it
    hp = hyperparams.HyperParameterHandler(off_cfg).get_hyper_params()
    stt.build_audio_processor(hp)
    reco = SpeechRecognizer(hp["language"])
    hp["char_map"], hp["char_map_length"] = reco.get_char_map(), reco.get_char_map_length()
    acoustic = stt._forward_model(hp, 1)
    assert acoustic.rescorer is None                                 # lm_weight 0: nothing of the language model is loaded
    acoustic.save(None, hp["checkpoint_dir"] + "/acoustic/")
    acoustic.close()

    plain = run_file(parent_cfg)
    assert plain.strip().startswith("[") and run_file(off_cfg) == plain       # lm_weight 0 prints what the parent prints

    # lm_weight > 0 without a language-model checkpoint: an error that names the directory
    with pytest.raises(RuntimeError) as ex:
        run_file(on_cfg)
    assert os.path.join(hp["checkpoint_dir"], "language") in str(ex.value)
    capsys.readouterr()

    lm = stt._language_model(hp, training=False)
    lm.save(None, hp["checkpoint_dir"])
    # the restored (untrained, nearly uniform) model barely changes the ranking; a SHARP one -- all its mass on the second distinct
    # hypothesis of the list -- flips the decoder's pick to that hypothesis
    seen = []

    def sharp(self, id_lists):
        seen.append([list(ids) for ids in id_lists])
        assert self.engine is not None and self.global_step.value == 0      # the restored model is the one asked
        return np.array([0.0 if k == 1 else -1000.0 for k in range(len(id_lists))])

    monkeypatch.setattr(LanguageModel, "score", sharp)
    flipped = run_file(on_cfg)
    assert len(seen) == 1 and len(seen[0]) >= 2 and len({tuple(c) for c in seen[0]}) == len(seen[0])      # one call, duplicates dropped
    first, second = (labels.get_labels_str(hp["char_map"], c) for c in seen[0][:2])
    assert plain == str([first]) + "\n"
    assert flipped == str([second]) + "\n" and flipped != plain


def test_train_language_from_the_command_line(tmp_path, monkeypatch):
    import stt
    from rnn_speech_amd.language_model import LanguageModel
    d = str(tmp_path)
    text = os.path.join(d, "sentences.txt")
    with open(text, "w") as fh:
        fh.write("\n".join(STUB_TRAIN * 5 + ["the yellow quick fox", "the green lazy fox"]) + "\n")
    cfg = os.path.join(d, "config.ini")
    with open(cfg, "w") as fh:
        fh.write(CONFIG % {"dir": d, "lm": LM_SECTION % {"text": text, "weight": "0"}})
    monkeypatch.setattr(sys, "argv", ["stt.py", "--train_language", "--config", cfg, "--max_epoch", "1"])
    stt.main()
    z = np.load(LanguageModel.checkpoint_path(os.path.join(d, "ckpt")))
    assert int(z["global_step"]) >= 2 and z["Output_layer/output_w"].shape == (32, 80)
