"""Engine(conv=...) against the float64 oracle -- oracle.model on the reference convolution's output with model lengths
(tests/conv_front_ref.py: model_oracle) -- with the tolerances of tests/test_gpu_model.py::test_forward_backward_adam_parity:
logits, loss and every gradient tensor, conv_w / conv_b included; dropout on with the library's own masks; once under the lookahead
convolution, once bidirectional.  Then the config.ini drop-in the way stt.py builds it, and the layer switched off."""
import os
import sys
import wave

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv_front_ref as ref  # noqa: E402
import lookahead_ref as la_ref  # noqa: E402

pytestmark = pytest.mark.gpu

from oracle import model as om  # noqa: E402  (checker only)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def rel_err(a, b):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-30))


def engine_masks(ws, L):
    """(in_masks, out_masks) as float64 numpy [T,B,H] per layer, exported by the library for the descriptor of `ws`
    (tests/test_gpu_dropout_oracle.py: engine_masks)."""
    from rnn_speech_amd import ops
    ins = [ops.lstm_dropout_multipliers(ws, "in", l).cpu().numpy().astype(np.float64) for l in range(L)]
    outs = [ops.lstm_dropout_multipliers(ws, "out", l).cpu().numpy().astype(np.float64) for l in range(L)]
    return ins, outs


def _engine(cfg):
    """An engine for a model config with the reference's filter bank, random biases (and taps), and its parameters as float32 numpy."""
    from rnn_speech_amd.engine import Engine
    _, L, H, B, T, U, mode, _, seed = cfg
    eng = Engine(L, H, ref.CONV_MODEL[5] * 40, ref.NUM_LABELS, B, T, U, seed=seed, conv=ref.CONV_MODEL,
                 lookahead=ref.LOOKAHEAD_CONTEXT if mode == "lookahead" else 0, bidirectional=mode == "bidirectional")
    rng = np.random.RandomState(seed + 1)
    p = eng.to_numpy()
    for k in p:
        if p[k].ndim == 1:
            p[k] = (rng.randn(*p[k].shape) * 0.1).astype(np.float32)
    if mode == "lookahead":
        p["lookahead_w"] = (rng.randn(ref.LOOKAHEAD_CONTEXT + 1, H) / 2.0).astype(np.float32)
    p["conv_w"], p["conv_b"] = ref.conv_params(cfg)
    eng.load_numpy(p)
    return eng, p


def _oracle_run(cfg, dense, masks):
    """run(p, x_model, model_lengths) -> (logits, loss, grads): the unchanged oracle of the model behind the convolution."""
    _, L, H, B, T, U, mode, _, _ = cfg
    C = ref.NUM_LABELS

    def plain(p, xm, Lo):
        im, omk = masks if masks is not None else (None, None)
        logits, _, cache = om.forward(p, xm, Lo, L, keep_cache=True, in_masks=im, out_masks=omk)
        loss, dl = om.ctc_loss_and_grad(logits, om.sparsify_labels(dense, C), Lo)
        return logits, loss, om.backward(p, cache, dl, Lo, L, in_masks=im, out_masks=omk)

    def lookahead(p, xm, Lo):
        return la_ref.model_oracle(om, p, xm, Lo, dense, L, C)

    def bidirectional(p, xm, Lo):
        logits, cache = om.forward_bidirectional(p, xm, Lo, L)
        loss, dl = om.ctc_loss_and_grad(logits, om.sparsify_labels(dense, C), Lo)
        return logits, loss, om.backward_bidirectional(p, cache, dl, Lo, L)

    return {"plain": plain, "lookahead": lookahead, "bidirectional": bidirectional}[mode]


@pytest.mark.parametrize("cfg", ref.MODEL_CONFIGS, ids=[c[0] for c in ref.MODEL_CONFIGS])
def test_forward_backward_parity_with_the_front_convolution(cfg):
    from rnn_speech_amd import ops
    _, L, H, B, T, U, mode, dropout, seed = cfg
    C, kt, kf, st, sf, G = ref.CONV_MODEL
    eng, p = _engine(cfg)
    x, lengths, dense = ref.model_batch(cfg)
    dx, dlen, dlab = torch.as_tensor(x).cuda(), torch.as_tensor(lengths).cuda(), torch.as_tensor(dense).cuda()
    To, W = ops.conv2d_out_shape(T, 40, C, st, sf)
    assert (eng.T, eng.D, eng.T_in, eng.D_in) == (To, W, T, G * 40) and eng.logits.shape == (To, B, ref.NUM_LABELS)
    assert eng.layout.names()[-2:] == ["conv_w", "conv_b"]

    with eng.on_stream():
        eng.zero_grads()
        if dropout:
            eng.mini_batch(dx, dlen, dlab, 0.8, 0.5, seed=4242)
        else:
            eng.mini_batch(dx, dlen, dlab)
    torch.cuda.synchronize()
    eng.check()
    path = eng.kernel_path()
    assert path["conv"] == C and path["run_length"] == To, path
    assert path["lookahead"] == (ref.LOOKAHEAD_CONTEXT if mode == "lookahead" else 0)
    Lo = ref.model_lengths(lengths, T, st)
    assert np.array_equal(eng.model_lengths(dlen).cpu().numpy(), Lo)
    masks = engine_masks(eng._ws, L) if dropout else None
    y_dev = eng.cv_y[:To].cpu().numpy()

    p64 = {k: v.astype(np.float64) for k, v in p.items()}
    k_pad = ops.conv2d_plan(T, B, G, 40, C, kt, kf, st, sf)["k_pad"]
    logits_ref, loss_ref, g_ref, y_ref, _ = ref.model_oracle(_oracle_run(cfg, dense, masks), p64, x, lengths, k_pad, y_dev)
    assert rel_err(y_dev, y_ref) < 1e-5
    logits = eng.logits.cpu().numpy()
    assert rel_err(logits, logits_ref) < 1e-4
    np.testing.assert_allclose(eng.loss.cpu().numpy(), loss_ref, rtol=1e-3, atol=1e-5)
    g = eng.to_numpy(eng.grads)
    assert sorted(g) == sorted(g_ref)
    for k in g_ref:
        print(k, "%.3g" % rel_err(g[k], g_ref[k]))
        assert rel_err(g[k], g_ref[k]) < 2e-3, (k, rel_err(g[k], g_ref[k]))
    assert np.abs(g_ref["conv_w"]).max() > 0 and np.abs(g_ref["conv_b"]).max() > 0
    # the greedy decoder reads model frames and model lengths
    ids, out_len = ops.ctc_greedy_decode(eng.logits, eng.model_lengths(dlen))
    ref_ids = om.greedy_decode(logits_ref, Lo)
    ids, out_len = ids.cpu().numpy(), out_len.cpu().numpy()
    for b in range(B):
        assert list(ids[b, :out_len[b]]) == ref_ids[b]


def test_run_length_clamp_counts_model_frames():
    """A batch whose longest row is shorter than the padded length: max_len arrives in source frames, the run is ceil(that / st)
    model frames, the convolution reads only the source frames behind them, and the gradients are those of the full run."""
    cfg = ("clamp", 2, 128, 4, 53, 6, "plain", False, 21)
    eng, p = _engine(cfg)
    x, _, dense = ref.model_batch(cfg)
    lengths = np.asarray([31, 0, 17, 30], np.int32)
    dx, dlen, dlab = torch.as_tensor(x).cuda(), torch.as_tensor(lengths).cuda(), torch.as_tensor(dense).cuda()
    dx[31:] = float("nan")                              # nothing past the longest row is read, at either run length
    out = []
    for max_len, run in ((None, 27), (31, 16)):
        eng.zero_grads()
        eng.mini_batch(dx, dlen, dlab, max_len=max_len)
        torch.cuda.synchronize()
        assert eng.kernel_path()["run_length"] == run
        assert list(eng.model_lengths(dlen).cpu().numpy()) == [16, 0, 9, 15]
        out.append((eng.logits.cpu().numpy().copy(), eng.to_numpy(eng.grads)))
    assert np.isfinite(out[0][0]).all() and np.isfinite(out[1][0]).all()
    assert rel_err(out[1][0], out[0][0]) < 1e-6
    for k in out[0][1]:
        assert rel_err(out[1][1][k], out[0][1][k]) < 1e-5, k


def test_layer_off_leaves_nothing_of_it(tmp_path, monkeypatch):
    """The default: no parameter, no buffer, no launch, and the checkpoint is byte for byte the one of a store that has never heard
    of the layer."""
    from rnn_speech_amd import checkpoint, ops
    from rnn_speech_amd.engine import Engine, ParamLayout, ParamStore
    L, H, D, C, B, T, U = 2, 32, 20, 30, 3, 24, 6
    eng = Engine(L, H, D, C, B, T, U, seed=3)
    assert eng.conv is None and (eng.T, eng.D, eng.T_in, eng.D_in) == (T, D, T, D)
    assert not [n for n in eng.layout.names() if n.startswith("conv")]
    assert not [a for a in vars(eng) if a.startswith("cv_")]
    assert eng.layout.slots == ParamLayout(L, H, D, C).slots

    def never(*a, **kw):
        raise AssertionError("the front convolution was launched with the layer off")

    monkeypatch.setattr(ops, "conv2d_fwd", never)
    monkeypatch.setattr(ops, "conv2d_bwd", never)
    rng = np.random.RandomState(0)
    x = torch.as_tensor(rng.randn(T, B, D).astype(np.float32)).cuda()
    n = torch.as_tensor(np.asarray([24, 11, 0], np.int32)).cuda()
    dense = np.zeros((B, U), np.int32)
    dense[:, 0], dense[:, 1] = 3, C - 1
    eng.zero_grads()
    eng.mini_batch(x, n, torch.as_tensor(dense).cuda())
    torch.cuda.synchronize()
    eng.check()
    assert eng.kernel_path()["conv"] == 0 and eng.model_lengths(n) is n
    eng.apply(3e-4, 1.0)
    plain = ParamStore(ParamLayout(L, H, D, C), "cpu")
    for a, b in ((plain.params, eng.params), (plain.adam_m, eng.adam_m), (plain.adam_v, eng.adam_v)):
        a.copy_(b.cpu())
    plain.adam_step = eng.adam_step
    pa, pb = str(tmp_path / "a.npz"), str(tmp_path / "b.npz")
    checkpoint.write(pa, checkpoint.pack(eng, 1, 1e-3))
    checkpoint.write(pb, checkpoint.pack(plain, 1, 1e-3))
    assert open(pa, "rb").read() == open(pb, "rb").read()


def test_engine_refuses_sizes_outside_the_ranges():
    from rnn_speech_amd.engine import Engine
    for conv, why in (((24, 3, 3, 1, 1, 1), "conv_channels"), ((32, 4, 3, 1, 1, 1), "odd"), ((32, 3, 3, 5, 1, 1), "each 1 .. 4"),
                      ((64, 3, 3, 1, 1, 1), "more than 4096"), ((32, 3, 3, 1, 1, 7), "feature groups")):
        with pytest.raises(ValueError, match=why):
            Engine(1, 16, 120, 30, 2, 12, 6, conv=conv)


# ---- the drop-in
def _write_wav(path, seed, seconds, sr=22050):
    rng = np.random.RandomState(seed)
    t = np.arange(int(seconds * sr)) / float(sr)
    sig = 0.05 * rng.randn(len(t)) + 0.3 * np.sin(2 * np.pi * (200 + 50 * seed) * t)
    with wave.open(path, "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(sr)
        w.writeframes((np.clip(sig, -1, 1) * 32767).astype("<i2").tobytes())


def test_drop_in_from_config(tmp_path, capsys):
    """conv_channels : 32 (kernel 11, 21, stride 2, 2) on fbank features in config.ini reach the engine the way stt.py builds it: one
    training step, --file's process_input, --align and the times it prints."""
    import stt
    from models.AcousticModel import Session
    from models.SpeechRecognizer import SpeechRecognizer
    from util.hyperparams import read_config_file
    src = open(os.path.join(ROOT, "config.ini")).read()
    src = src.replace("checkpoint_dir", "checkpoint_dir : %s\n#" % (tmp_path / "ckpt"), 1)
    for old, new in (("conv_channels : 0", "conv_channels : 32"), ("signal_processing : mfcc", "signal_processing : fbank"),
                     ("max_input_seq_length : 1001", "max_input_seq_length : 90"), ("max_target_seq_length : 161", "max_target_seq_length : 12"),
                     ("num_layers : 3", "num_layers : 2"), ("hidden_size : 512", "hidden_size : 64"), ("batch_size : 32", "batch_size : 2"),
                     ("train_decoder : beam", "train_decoder : greedy")):
        assert old in src
        src = src.replace(old, new, 1)
    cfg = tmp_path / "config.ini"
    cfg.write_text(src)
    hp = read_config_file(str(cfg))
    assert (hp["conv_channels"], hp["conv_kernel"], hp["conv_stride"]) == (32, (11, 21), (2, 2))
    audio = stt.build_audio_processor(hp)
    reco = SpeechRecognizer(hp["language"])
    hp["char_map"], hp["char_map_length"] = reco.get_char_map(), reco.get_char_map_length()
    assert (hp["input_dim"], hp["out_seq_length"]) == (120, 90) and stt.conv_option(hp) == (32, 11, 21, 2, 2, 3)

    texts = ["hello there", "it'll do"]
    items = []
    for i, (txt, seconds) in enumerate(zip(texts, (0.6, 1.2))):         # the second recording is longer than 90 source frames
        path = str(tmp_path / ("u%d.wav" % i))
        _write_wav(path, i, seconds)
        items.append([path, txt, None])
    sess = Session()
    model, t_it, v_it = stt.build_acoustic_training_rnn(sess, hp, dict(tb_name=None, timeline=False, learn_rate=None), items, items[:1])
    try:
        eng = model.engine
        assert model.conv == (32, 11, 21, 2, 2, 3) and model.max_input_seq_length == 90
        assert (eng.T_in, eng.D_in, eng.T, eng.D, eng.B) == (90, 120, 45, 20 * 32, 2)
        assert eng.layout.slots["input_w"][1] == (640, 64) and eng.layout.slots["conv_w"][1] == (693, 32)
        (f1, n1, d1), = list(t_it.dataset.with_items(items).batches())
        assert tuple(f1.shape) == (90, 2, 120) and 40 < n1[0] < 90 <= n1[1]       # the second recording is truncated at 90
        want = [-(-min(int(n), 90) // 2) for n in n1]                             # model frames of the two rows
        loss, err, step, exhausted = model.run_train_step(sess, 1, 1.0)
        assert step == 1 and np.isfinite(loss)
        eng.check()
        path = eng.kernel_path()
        assert path["conv"] == 32 and path["run_length"] == 45, path
        assert sorted(eng.model_lengths(None).cpu().numpy()) == sorted(want)     # the model-frame counts
        # (the gradient buffer is only zeroed by the next start_batch: it still holds this step's contribution)
        assert float(eng.g("conv_w").abs().max()) > 0.0 and float(eng.g("conv_b").abs().max()) > 0.0
        # --file style: process_input on source frames and source lengths
        pred = model.process_input(sess, f1, n1)
        assert len(pred) == 2 and eng.kernel_path()["run_length"] == 45
        assert list(eng.model_lengths(None).cpu().numpy()) == want
        # the aligner works in model frames; model frame 1 is centred 2 hops into the file
        from util.dataprocessor import DataProcessor
        labels = [DataProcessor.get_str_labels(hp["char_map"], DataProcessor.clean_label(t), add_eos=False) for t in texts]
        spans = model.align(sess, f1, n1, labels)
        assert len(spans) == 2 and all(len(row) == len([v for v in lab if v != 0]) > 0 for row, lab in zip(spans, labels))
        for row, n in zip(spans, want):
            assert all(0 <= first <= last < n for _, first, last, _ in row)
        assert stt.frame_seconds(audio, model.conv) == 2 * audio.hop_samples / float(audio.load_sr)
    finally:
        model.close()
    # stt.py's own --file and --align on the first recording (a fresh forward model of batch 1 each)
    assert len(stt.process_file(audio, hp, items[0][0])) == 1
    words = stt.align_file(audio, hp, items[0][0], texts[0])
    assert [w[0] for w in words] == ["hello", "there"]
    frame_s = 2 * audio.hop_samples / float(audio.load_sr)
    lines = [ln.split() for ln in capsys.readouterr().out.splitlines() if ln.endswith(" hello") or ln.endswith(" there")]
    assert len(lines) == 2
    for (word, first, last, conf), ln in zip(words, lines):
        assert 0 <= first <= last < want[0]
        assert ln[0] == "%.3f" % (first * frame_s) and ln[1] == "%.3f" % (last * frame_s)
