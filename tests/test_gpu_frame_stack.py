"""Low frame rate input on the GPU (csrc/frame_stack.hip): the kernel bit for bit against tests/frame_stack_ref.py at the edges,
through the front end, through the model against the float64 oracle, and as a config.ini drop-in the way stt.py builds it."""
import os
import sys
import wave

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import model as om  # noqa: E402  (checker only)

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import frame_stack_ref as ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bits(t):
    return t.cpu().numpy().view(np.uint32)


# ------------------------------------------------------------------------------------------------ 1. exact copy at the edges
@pytest.mark.parametrize("name", sorted(ref.CASES))
def test_exact_copy_at_the_edges(name):
    """uint32 bit patterns, np.array_equal: no tolerance, it is a copy.  `out` starts as a sentinel (every element must be written),
    the source holds a NaN at every frame at or past its row's length (the kernel masks by the length and must not pass them on),
    the valid region carries -0.0, a denormal, +-inf and a NaN payload."""
    from rnn_speech_amd import ops
    k, s, D, t_in, B, _, fields = ref.CASES[name]
    plan = ops.frame_stack_plan(B, D, t_in, k, s)
    assert plan == ref.expected_plan(B, D, t_in, k, s)
    assert plan["vec"] == (4 if D % 4 == 0 else 1) and all(plan[f] == v for f, v in fields.items()), plan
    x, lengths = ref.case_inputs(name)
    want, want_n = ref.stack(x, lengths, k, s)
    dx = torch.from_numpy(x.view(np.float32)).cuda()
    assert np.array_equal(bits(dx), x)                                  # the upload keeps the patterns
    out = torch.from_numpy(np.full(want.shape, ref.SENTINEL, np.uint32).view(np.float32)).cuda()
    got, got_n = ops.frame_stack(dx, [int(n) for n in lengths], k, s, out=out)
    torch.cuda.synchronize()
    assert got is out and got.shape == (plan["t_out"], B, plan["d_out"])
    g = bits(got)
    assert not np.any(g == ref.SENTINEL), "elements of out left unwritten"
    assert not np.any(g == ref.POISON), "frames at or past a row's length reached the result"
    assert np.array_equal(g, want)
    assert list(got_n) == list(want_n)
    assert np.array_equal(bits(dx), x)                                  # the source is untouched


# ------------------------------------------------------------------------------------------------ 2. through the front end
def _synth(seed, n, sr=16000):
    rng = np.random.RandomState(seed)
    t = np.arange(n) / float(sr)
    return (0.1 * rng.randn(n) + 0.3 * np.sin(2 * np.pi * 300 * (1 + seed % 5) * t)).astype(np.float32)


def test_through_the_front_end():
    from rnn_speech_amd import ops
    from util.audioprocessor import AudioProcessor
    sr, T = 16000, 60
    signals = [_synth(1, 4000), _synth(2, 7333), _synth(3, 11000)]         # 26, 46 and 69 frames: one row is truncated at T
    plain = AudioProcessor(T, "mfcc", n_mfcc=40, load_sr=sr)
    lfr = AudioProcessor(T, "mfcc", n_mfcc=40, load_sr=sr, frame_stack=3, frame_skip=3)
    feat, n = plain.process_batch(signals, sr)
    got, got_n = lfr.process_batch(signals, sr)
    assert max(n) > T > min(n)
    want, want_n = ref.stack(bits(feat), n, 3, 3)
    assert got.shape == (lfr.out_seq_length, 3, lfr.feature_size) == (20, 3, 120)
    assert np.array_equal(bits(got), want)
    assert list(got_n) == list(want_n) == [-(-v // 3) for v in n]
    # the reference surface: [n, feature_size] of the first row, its untruncated length
    one, one_n = lfr.process_signal(signals[0], sr)
    src_one, src_n = plain.process_signal(signals[0], sr)
    want_one, _ = ref.stack(src_one.view(np.uint32)[:, None, :], [src_n], 3, 3)
    assert one_n == got_n[0] == 9 and one.shape == (9, 120) and np.array_equal(one.view(np.uint32), want_one[:, 0])
    # (1, 1): the front end's own tensor -- nothing is copied, nothing is launched
    seen = {}
    real = ops.frontend

    def spy(*a, **kw):
        seen["feat"], seen["n"] = real(*a, **kw)
        return seen["feat"], seen["n"]

    ops.frontend = spy
    try:
        same, same_n = plain.process_batch(signals, sr)
    finally:
        ops.frontend = real
    assert same is seen["feat"] and same_n is seen["n"]


# ------------------------------------------------------------------------------------------------ 3. through the model
def test_through_the_model():
    """Engine(2, 128, 120, 80, 20, 10, 3) on ops.frame_stack of a random [30, 20, 40] source at (3, 3) against oracle.model on the
    numpy-stacked float64 input.  Tolerances: tests/test_gpu_model.py::test_forward_backward_adam_parity's, unchanged."""
    from rnn_speech_amd import ops
    from rnn_speech_amd.engine import Engine
    L, H, D, C, B, T, U = 2, 128, 120, 80, 20, 10, 3
    eng = Engine(L, H, D, C, B, T, U, seed=7)
    rng = np.random.RandomState(5)
    p = eng.to_numpy()
    for key in p:                               # non-zero biases exercise the bias paths
        if p[key].ndim == 1:
            p[key] = (rng.randn(*p[key].shape) * 0.1).astype(np.float32)
    eng.load_numpy(p)
    src = rng.randn(30, B, 40).astype(np.float32)
    src_len = rng.randint(21, 31, size=B).astype(np.int32)
    dense = np.zeros((B, U), np.int32)
    for b in range(B):
        n = rng.randint(1, U)
        dense[b, :n] = rng.randint(1, C - 1, size=n)
        dense[b, n] = C - 1
    x64, lengths = ref.stack(src.astype(np.float64), src_len, 3, 3)
    lengths = lengths.astype(np.int32)
    assert x64.shape == (T, B, D) and lengths.min() >= 2 * U + 1 == 7 and lengths.max() <= T      # every row has a feasible alignment

    dx, dn = ops.frame_stack(torch.as_tensor(src).cuda(), [int(v) for v in src_len], 3, 3)
    assert list(dn) == list(lengths) and np.array_equal(dx.cpu().numpy(), x64.astype(np.float32))

    p64 = {key: v.astype(np.float64) for key, v in p.items()}
    logits_ref, _, cache = om.forward(p64, x64, lengths, L, keep_cache=True)
    loss_ref, dl_ref = om.ctc_loss_and_grad(logits_ref, om.sparsify_labels(dense, C), lengths)
    g_ref = om.backward(p64, cache, dl_ref, lengths, L)
    assert np.all(np.isfinite(loss_ref)) and np.all(loss_ref > 0)

    eng.zero_grads()
    eng.mini_batch(dx, torch.as_tensor(lengths).cuda(), torch.as_tensor(dense).cuda())
    torch.cuda.synchronize()
    eng.check()

    def rel_err(a, b):
        a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
        return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-30))

    assert rel_err(eng.logits.cpu().numpy(), logits_ref) < 1e-4
    np.testing.assert_allclose(eng.loss.cpu().numpy(), loss_ref, rtol=1e-3, atol=1e-5)
    g = eng.to_numpy(eng.grads)
    assert set(g_ref) <= set(g)
    for key in g_ref:
        assert rel_err(g[key], g_ref[key]) < 2e-3, key


# ------------------------------------------------------------------------------------------------ 4. drop-in
def _write_wav(path, seed, seconds, sr=22050):
    rng = np.random.RandomState(seed)
    t = np.arange(int(seconds * sr)) / float(sr)
    sig = 0.05 * rng.randn(len(t)) + 0.3 * np.sin(2 * np.pi * (200 + 50 * seed) * t)
    with wave.open(path, "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(sr)
        w.writeframes((np.clip(sig, -1, 1) * 32767).astype("<i2").tobytes())


def test_drop_in_from_config(tmp_path):
    """frame_stack : 3, frame_skip : 3, max_input_seq_length : 90 in config.ini reach the processor, the datasets and the engine the
    way stt.py builds them; one train step, the feature cache, the aligner and the time --align prints."""
    import stt
    from models.AcousticModel import Session
    from models.SpeechRecognizer import SpeechRecognizer
    from util.hyperparams import read_config_file
    src = open(os.path.join(ROOT, "config.ini")).read()
    src = src.replace("checkpoint_dir", "checkpoint_dir : %s\n#" % (tmp_path / "ckpt"), 1)
    for old, new in (("frame_stack : 1", "frame_stack : 3"), ("frame_skip : 1", "frame_skip : 3"),
                     ("max_input_seq_length : 1001", "max_input_seq_length : 90"), ("max_target_seq_length : 161", "max_target_seq_length : 12"),
                     ("num_layers : 3", "num_layers : 2"), ("hidden_size : 512", "hidden_size : 64"), ("batch_size : 32", "batch_size : 2"),
                     ("n_mfcc : 40", "n_mfcc : 20"), ("feature_cache_mb : 0", "feature_cache_mb : 4"), ("train_decoder : beam", "train_decoder : greedy")):
        assert old in src
        src = src.replace(old, new, 1)
    cfg = tmp_path / "config.ini"
    cfg.write_text(src)
    hp = read_config_file(str(cfg))
    assert (hp["frame_stack"], hp["frame_skip"], hp["max_input_seq_length"]) == (3, 3, 90)
    audio = stt.build_audio_processor(hp)
    reco = SpeechRecognizer(hp["language"])
    hp["char_map"], hp["char_map_length"] = reco.get_char_map(), reco.get_char_map_length()
    assert (hp["input_dim"], hp["out_seq_length"]) == (60, 30) and audio.feature_size == 3 * audio.source_feature_size

    texts = ["hello there", "it'll do"]
    items = []
    for i, (txt, seconds) in enumerate(zip(texts, (0.6, 1.2))):         # 61 and 121 source frames: the second is truncated at 90
        path = str(tmp_path / ("u%d.wav" % i))
        _write_wav(path, i, seconds)
        items.append([path, txt, None])
    sess = Session()
    model, t_it, v_it = stt.build_acoustic_training_rnn(sess, hp, dict(tb_name=None, timeline=False, learn_rate=None), items, items[:1])
    try:
        eng = model.engine
        assert (eng.D, eng.T, eng.B) == (3 * 20, 30, 2)
        assert (model.frame_stack, model.frame_skip, model.max_input_seq_length) == (3, 3, 30)
        train = t_it.dataset
        assert (train.T, train.audio.frame_stack, train.audio.frame_skip) == (30, 3, 3)
        loss, err, step, exhausted = model.run_train_step(sess, 1, 1.0)
        assert step == 1 and np.isfinite(loss)
        eng.check()

        # the same batch a second time comes out of the feature cache and is the same batch, bit for bit
        assert set(train._cache) == {items[0][0], items[1][0]}
        fresh = stt.AcousticModel.build_dataset(items, 2, 90, 12, "mfcc", hp["char_map"], n_mfcc=20, frame_stack=3, frame_skip=3)
        (f0, n0, d0), = list(fresh.batches())
        (f1, n1, d1), = list(train.with_items(items).batches())
        assert f0.shape == (30, 2, 60) and list(n0) == list(n1) == [21, 41] and np.array_equal(d0, d1)
        assert np.array_equal(bits(f0), bits(f1))
        plain = stt.AcousticModel.build_dataset(items, 2, 90, 12, "mfcc", hp["char_map"], n_mfcc=20)
        (fp, np_, _), = list(plain.batches())
        want, want_n = ref.stack(bits(fp), np_, 3, 3)
        assert np.array_equal(bits(f0), want) and list(n0) == list(want_n)

        # the aligner works in model frames; frame 1 starts 3 hops into the file
        from util.dataprocessor import DataProcessor
        labels = [DataProcessor.get_str_labels(hp["char_map"], DataProcessor.clean_label(t), add_eos=False) for t in texts]
        spans = model.align(sess, f1, np.minimum(n1, 30), labels)
        assert len(spans) == 2 and all(len(row) == len([v for v in lab if v != 0]) > 0 for row, lab in zip(spans, labels))
        for row, n in zip(spans, np.minimum(n1, 30)):
            assert all(0 <= first <= last < n <= 30 for _, first, last, _ in row)
        assert stt.frame_seconds(audio) * 1 == 3 * audio.hop_samples / float(audio.load_sr)
        assert audio.frame_hop_samples == 3 * 220
    finally:
        model.close()
