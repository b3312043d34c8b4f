"""The transducer model on the GPU (rnn_speech_amd/transducer.py): loss and every gradient tensor of one mini-batch against the
float64 oracle (oracle.model for the two LSTM networks, transducer_ref for the joint and the lattice), a wrong-target control,
optimiser steps, checkpoints to the bit, greedy decoding against the reference decoder, objective : ctc untouched, and stt.py end
to end with objective : transducer.  Small model: 2 x 128 encoder, 1 x 128 prediction network, J 64, C 80, B 3, T 24, U 9."""
import os
import sys
import wave

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lm_fusion_ref as F  # noqa: E402
import transducer_ref as R  # noqa: E402
from oracle import model as om  # noqa: E402

pytestmark = pytest.mark.gpu

L, H, D, C, B, T, U, J, LP, HP = 2, 128, 20, 80, 3, 24, 9, 64, 1, 128
LENGTHS = np.array([24, 17, 20], np.int32)


def _engine(seed=11):
    from rnn_speech_amd.transducer import TransducerEngine
    return TransducerEngine(L, H, D, C, B, T, U, joint_size=J, pred_layers=LP, pred_hidden=HP, seed=seed)


def _batch(wrong=False):
    rng = np.random.RandomState(0)
    x = rng.randn(T, B, D).astype(np.float32)
    dense = np.zeros((B, U), np.int32)
    dense[0, :6] = [5, 6, 6, 7, 0, 79]
    dense[1, :1] = [79]                                            # an empty target
    dense[2, :9] = [1, 2, 3, 4, 5, 6, 7, 8, 9]                    # U labels, no room for the EOS
    if wrong:                                                      # (other labels AND other counts: at a fresh model, whose rows are
        dense[0, :6] = [9, 79, 0, 0, 0, 0]                         # near uniform, one swapped label alone moves the loss by 0.1 %)
        dense[2, 2:] = 0
        dense[2, 2] = 79
    return x, dense


def _part(eng, prefix):
    return {k[len(prefix):]: v.astype(np.float64) for k, v in eng.to_numpy().items() if k.startswith(prefix)}


def _oracle(eng, x, dense, enc_masks=(None, None), pred_masks=(None, None)):
    """float64 (loss [B], gradients under the store's names) of the mini-batch at the engine's parameters; the (in, out) dropout
    multipliers of the two stacks as read back from the library, or none."""
    pe, pp = _part(eng, "encoder/"), _part(eng, "prediction/")
    all_p = {k: v.astype(np.float64) for k, v in eng.to_numpy().items()}
    targets, n, tok, tok_len = R.targets_ref(dense, C)
    f, _, ce = om.forward(pe, x.astype(np.float64), LENGTHS, L, keep_cache=True, in_masks=enc_masks[0], out_masks=enc_masks[1])
    onehot = np.zeros((U + 1, B, C))
    for b in range(B):
        for t in range(tok_len[b]):
            onehot[t, b, tok[b, t]] = 1.0
    g, _, cp = om.forward(pp, onehot, tok_len, LP, keep_cache=True, in_masks=pred_masks[0], out_masks=pred_masks[1])
    logits = R.joint_ref(f, g, all_p["joint_w"], all_p["joint_b"])
    loss, dl = R.loss_ref(logits, targets, n, LENGTHS)
    live = R.live_mask(LENGTHS, n, T, U)
    (df, dg, dw, db), _ = R.joint_bwd_ref(dl, f, g, all_p["joint_w"], live)
    grads = {"joint_w": dw, "joint_b": db}
    grads.update({"encoder/" + k: v for k, v in om.backward(pe, ce, df, LENGTHS, L, in_masks=enc_masks[0], out_masks=enc_masks[1]).items()})
    grads.update({"prediction/" + k: v for k, v in om.backward(pp, cp, dg, tok_len, LP, in_masks=pred_masks[0], out_masks=pred_masks[1]).items()})
    return loss, grads


def _run(eng, x, dense, **kw):
    eng.zero_grads()
    with eng.on_stream():
        eng.mini_batch(torch.as_tensor(x).cuda(), torch.as_tensor(LENGTHS).cuda(), torch.as_tensor(dense).cuda(), **kw)
    torch.cuda.synchronize()
    eng.check()
    return eng.loss.cpu().numpy().astype(np.float64), {k: v.astype(np.float64) for k, v in eng.to_numpy(eng.grads).items()}


def test_loss_and_every_gradient_tensor_equal_the_float64_oracle_and_a_wrong_target_does_not():
    eng = _engine()
    x, dense = _batch()
    want_loss, want = _oracle(eng, x, dense)
    loss, grads = _run(eng, x, dense)
    print("loss", loss, want_loss)
    assert np.allclose(loss, want_loss, rtol=1e-3, atol=1e-5)
    assert sorted(grads) == sorted(want) == sorted(eng.layout.names())
    for k in sorted(want):
        err, top = np.abs(grads[k] - want[k]).max(), np.abs(want[k]).max()
        print("%-28s max %.3e  error / max %.2e" % (k, top, err / top))
        assert top > 0 and err <= 2e-3 * top, k
    path = eng.kernel_path()
    assert path["objective"] == "transducer" and not path["fused_ctc_head"] and path["run_length"] == T
    # the control: the same comparison against the oracle of ANOTHER target misses by far
    other_loss, other = _oracle(eng, x, _batch(wrong=True)[1])
    assert (np.abs(loss - other_loss)[[0, 2]] > 1e-2 * np.abs(other_loss)[[0, 2]]).all()
    assert np.abs(grads["joint_w"] - other["joint_w"]).max() > 1e-2 * np.abs(other["joint_w"]).max()
    # a shorter run length (the longest row, known to the host) gives the same loss
    loss_short, _ = _run(eng, x, dense, max_len=int(LENGTHS.max()))
    assert np.allclose(loss_short, want_loss, rtol=1e-3, atol=1e-5)


def test_dropout_on_the_same_check_with_the_masks_of_both_stacks_read_back():
    from test_gpu_dropout_oracle import engine_masks
    eng = _engine()
    x, dense = _batch()
    keep = dict(keep_in=0.8, keep_out=0.5, seed=7)
    loss, grads = _run(eng, x, dense, **keep)
    # (the descriptors still hold this step's keep probabilities and seeds: the encoder's `seed`, the prediction network's `seed + 1`)
    enc_masks, pred_masks = engine_masks(eng.encoder._ws, L), engine_masks(eng.prediction._ws, LP)
    for masks in (enc_masks, pred_masks):
        for m, k in zip(masks, (0.8, 0.5)):
            vals = np.unique(np.round(np.concatenate([a.ravel() for a in m]), 6))
            assert list(vals) == [0.0, round(1.0 / k, 6)], vals                  # inverted dropout at the keep probability handed in
    assert not np.array_equal(enc_masks[1][0][:U + 1], pred_masks[1][0])         # the two stacks draw from different seeds
    want_loss, want = _oracle(eng, x, dense, enc_masks, pred_masks)
    print("loss", loss, want_loss)
    assert np.allclose(loss, want_loss, rtol=1e-3, atol=1e-5)
    for k in sorted(want):
        err, top = np.abs(grads[k] - want[k]).max(), np.abs(want[k]).max()
        print("%-28s max %.3e  error / max %.2e" % (k, top, err / top))
        assert top > 0 and err <= 2e-3 * top, k
    # and the masks matter: the dropout-off oracle misses
    off_loss, off = _oracle(eng, x, dense)
    assert not np.isclose(loss, off_loss, rtol=1e-3, atol=1e-5).any()         # (every row misses the parity tolerance itself)
    assert np.abs(grads["prediction/kernel_0"] - off["prediction/kernel_0"]).max() > 1e-2 * np.abs(off["prediction/kernel_0"]).max()
    # a forward-only mini-batch with the same keep probabilities and seed draws the same masks: the same loss, no gradient added
    before = eng.grads.clone()
    with eng.on_stream():
        eng.mini_batch(torch.as_tensor(x).cuda(), torch.as_tensor(LENGTHS).cuda(), torch.as_tensor(dense).cuda(), compute_gradients=False, **keep)
    torch.cuda.synchronize()
    eng.check()
    assert np.allclose(eng.loss.cpu().numpy(), want_loss, rtol=1e-3, atol=1e-5) and torch.equal(before, eng.grads)


def test_a_few_optimiser_steps_lower_the_loss_and_save_and_restore_reproduce_the_store_to_the_bit(tmp_path):
    from rnn_speech_amd import checkpoint
    eng = _engine()
    x, dense = _batch()
    first, _ = _run(eng, x, dense)
    for _ in range(5):
        eng.apply(1e-2, 5.0)
        last, _ = _run(eng, x, dense, keep_in=0.9, keep_out=0.9, seed=3)
    eng.apply(1e-2, 5.0)
    torch.cuda.synchronize()
    last, _ = _run(eng, x, dense)
    print("loss", first.sum(), "->", last.sum())
    assert last.sum() < 0.9 * first.sum() and np.isfinite(last).all()
    eng.apply(1e-2, 5.0)
    path = str(tmp_path / "t.npz")
    checkpoint.write(path, checkpoint.pack(eng, 7, 1e-2))
    z = np.load(path)
    assert "Encoder/Output_layer/output_w" in z and "Prediction/Input_Layer/input_w" in z and "Joint_Layer/joint_w" in z
    assert "adam/m/Prediction/rnn/multi_rnn_cell/cell_0/basic_lstm_cell/kernel" in z
    other = _engine(seed=99)
    assert checkpoint.unpack(z, other) == (7, float(np.float32(1e-2)), True)
    assert other.adam_step == eng.adam_step == 7
    for a, b in ((eng.params, other.params), (eng.adam_m, other.adam_m), (eng.adam_v, other.adam_v)):
        assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
    # the parts ARE slices of the one buffer: the encoder's and the prediction network's own stores see the restored values
    assert other.encoder.params.data_ptr() == other.params.data_ptr()
    assert other.prediction.p("output_w").cpu().numpy().tobytes() == eng.p("prediction/output_w").cpu().numpy().tobytes()


def test_greedy_decode_equals_the_reference_decoder_with_a_capped_row_and_an_empty_utterance():
    eng = _engine(seed=5)
    rng = np.random.RandomState(4)
    eng.p("joint_b").copy_(torch.as_tensor((rng.randn(C) * 0.5).astype(np.float32)))
    eng.p("joint_w").mul_(6.0)                                    # (decided rows: margins far above the float32 error)
    eng.p("joint_b")[C - 1] += 1.0
    x, _ = _batch()
    lengths = np.array([24, 0, 9], np.int32)
    dl = torch.as_tensor(lengths).cuda()
    with eng.on_stream():
        eng.forward(torch.as_tensor(x).cuda(), dl)
        ids, out_len = eng.greedy_decode(dl)
    torch.cuda.synchronize()
    eng.check()
    ids, out_len = ids.cpu().numpy(), out_len.cpu().numpy()
    allp = eng.to_numpy()
    pp = {k[len("prediction/"):]: v for k, v in allp.items() if k.startswith("prediction/")}
    p = dict(pp, pred_w=pp["output_w"], pred_b=pp["output_b"])
    p["output_w"], p["output_b"] = np.zeros((HP, C), np.float32), np.zeros(C, np.float32)      # (the step's own output layer: unused)
    f = eng.logits.cpu().numpy()
    args = (p, LP, f, lengths, U, allp["joint_w"], allp["joint_b"])
    want_ids, want_len, choices, rows64 = R.greedy_walk(*args, F.lm_step_ref)
    _, _, _, rows32 = R.greedy_walk(*args, F.lm_step_f32, dtype=np.float32, forced=choices)
    margin, err = R.greedy_margins(rows64, rows32)
    print("margin %.3e, float32 walk error %.3e, lengths" % (margin, err), want_len)
    assert margin > 2 * R.greedy_logit_bound(err)                 # (the case is decidable; tests/test_cpu_transducer.py holds the table's)
    assert list(out_len) == list(want_len) and want_len[1] == 0 and want_len.max() == U
    for b in range(B):
        assert list(ids[b, :out_len[b]]) == list(want_ids[b, :want_len[b]])


def test_objective_ctc_builds_a_plain_acoustic_model_and_loads_nothing_of_the_transducer(tmp_path):
    import subprocess
    code = ("import sys; sys.path.insert(0, %r); import stt; from models.AcousticModel import AcousticModel\n"
            "hp = dict(num_layers=1, hidden_size=32, max_input_seq_length=20, max_target_seq_length=6, input_dim=20,\n"
            "          batch_normalization=False, char_map_length=80, objective='ctc')\n"
            "m = stt._acoustic_model(hp, 2, True); assert type(m) is AcousticModel\n"
            "m.create_forward_rnn(); assert type(m.engine).__name__ == 'Engine'\n"
            "assert 'rnn_speech_amd.transducer' not in sys.modules; print('plain ok')\n" % os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "plain ok" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]


def test_what_the_transducer_does_not_do_is_refused_by_the_name_of_its_key():
    from rnn_speech_amd.transducer import TransducerModel, check_options
    for hp, word in (({"train_decoder": "beam"}, "train_decoder"), ({"lm_weight": 0.5}, "lm_weight"),
                     ({"decode_blank_skip": 0.9}, "decode_blank_skip")):
        with pytest.raises(ValueError, match=word):
            check_options(hp, training=True)
    check_options({"train_decoder": "beam"}, training=False)      # (a forward model does not read the key)
    m = TransducerModel(1, 32, 2, 20, 6, 20, False, 80)
    m.train_decoder = "beam"
    with pytest.raises(ValueError, match="train_decoder"):
        m.create_training_rnn(1.0, 1.0, 5, 1e-3, 0.5)
    m = TransducerModel(1, 32, 2, 20, 6, 20, False, 80)
    m.joint_size, m.pred_hidden = 32, 16
    m.create_forward_rnn()
    with pytest.raises(ValueError, match="--align"):
        m.align(None, np.zeros((20, 2, 20), np.float32), [20, 20], [[5], [6]])


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
objective : transducer
transducer_joint_size : 32
transducer_pred_hidden : 16

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
train_decoder : greedy

[logging]
log_level : WARNING
"""


def _write_wav(path, seed, seconds=0.5, sr=22050):
    rng = np.random.RandomState(seed)
    t = np.arange(int(seconds * sr)) / float(sr)
    sig = 0.05 * rng.randn(len(t)) + 0.3 * np.sin(2 * np.pi * (200 + 50 * seed) * t)
    with wave.open(path, "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(sr)
        w.writeframes((np.clip(sig, -1, 1) * 32767).astype("<i2").tobytes())


def test_stt_trains_and_transcribes_a_file_with_objective_transducer(tmp_path, monkeypatch, capsys):
    d = str(tmp_path)
    texts = ["hello there", "good bye", "it'll do", "yes", "no way", "well-being"]
    with open(os.path.join(d, "train.tsv"), "w") as tr, open(os.path.join(d, "test.tsv"), "w") as te:
        for i, txt in enumerate(texts):
            p = os.path.join(d, "u%d.wav" % i)
            _write_wav(p, i)
            (tr if i < 5 else te).write("%s\t%s\n" % (p, txt))
        te.write("%s\t%s\n" % (os.path.join(d, "u0.wav"), texts[0]))
    cfg = os.path.join(d, "config.ini")
    with open(cfg, "w") as fh:
        fh.write(CONFIG % {"dir": d})
    import stt
    monkeypatch.setattr(sys, "argv", ["stt.py", "--train_acoustic", "--config", cfg, "--max_epoch", "1"])
    stt.main()
    ckpt = os.path.join(d, "ckpt", "acoustic")
    z = np.load(os.path.join(ckpt, [f for f in os.listdir(ckpt) if f.endswith(".npz")][0]))
    assert "Joint_Layer/joint_w" in z and z["Joint_Layer/joint_w"].shape == (32, 80)
    assert z["Prediction/Input_Layer/input_w"].shape == (80, 16)
    capsys.readouterr()
    monkeypatch.setattr(sys, "argv", ["stt.py", "--file", os.path.join(d, "u1.wav"), "--config", cfg])
    stt.main()
    assert capsys.readouterr().out.strip().startswith("[")
