"""Feature normalisation on the GPU (csrc/feature_norm.hip): the kernels against tests/feature_norm_ref.py at the edges and within
the derived bound, global mode bit for bit, the moments and the corpus statistics in float64, through the front end, through the
model against the float64 oracle, and as a config.ini drop-in the way stt.py builds it."""
import os
import sys
import wave

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import model as om  # noqa: E402  (checker only)

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import feature_norm_ref as ref  # noqa: E402
import frame_stack_ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bits(t):
    return t.cpu().numpy().view(np.uint32)


def upload(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


# ------------------------------------------------------------------------------------------------ 1. the edges
@pytest.mark.parametrize("name", ref.GPU_CASES)
def test_edges(name):
    """Per case: the plan is the expected one; every word at or past a row's length is unchanged bit for bit (the planted NaN, and
    a finite word in a second run, whose valid frames must not depend on the padding either); the valid frames are within the
    derived bound of feature_norm_ref (worst ratio printed as a FEATNORM record); constant dims are exactly 0; a second call on a
    fresh copy gives identical bits; so does the call without variance normalisation against its own reference."""
    from rnn_speech_amd import ops
    D, t_in, B, _, fields = ref.CASES[name]
    plan = ops.feature_norm_plan(B, D, t_in, "utterance")
    assert plan == ref.expected_plan(B, D, t_in) and all(plan[f] == v for f, v in fields.items()), plan
    x, lengths = ref.case_inputs(name)
    n_frames = [int(n) for n in lengths]
    dx = upload(x)
    assert np.array_equal(bits(dx), x.view(np.uint32))                  # the upload keeps the patterns
    got = ops.feature_norm(dx, n_frames, "utterance")
    torch.cuda.synchronize()
    assert got is dx
    g = got.cpu().numpy()
    verdict = ref.judge(g, x, lengths, ref.const_dims(name))
    print("FEATNORM %s vec=%d split=%d wgs=%d worst_ratio=%.3f" % (name, plan["vec"], plan["split"], plan["workgroups"], verdict["ratio"]))
    assert verdict["pad_intact"], "words at or past a row's length were written"
    assert verdict["const_zero"], "a constant dim did not come out as exact zeros"
    assert verdict["ratio"] <= 1.0, verdict
    for b, n in enumerate(ref.clipped(lengths, t_in)):
        if n == 1:
            assert not g[0, b].any()                                    # one frame: zeros

    again = ops.feature_norm(upload(x), n_frames, "utterance")
    assert np.array_equal(bits(again), g.view(np.uint32))

    xf, _ = ref.case_inputs(name, ref.PAD_FINITE)                       # the same valid frames, finite padding
    gf = ops.feature_norm(upload(xf), n_frames, "utterance").cpu().numpy()
    for b, n in enumerate(ref.clipped(lengths, t_in)):
        assert np.all(gf[n:, b].view(np.uint32) == ref.PAD_FINITE)
        assert np.array_equal(gf[:n, b].view(np.uint32), g[:n, b].view(np.uint32))

    gm = ops.feature_norm(upload(x), n_frames, "utterance", norm_vars=False).cpu().numpy()
    only_mean = ref.judge(gm, x, lengths, ref.const_dims(name), norm_vars=False)
    assert ref.passes(only_mean), only_mean


def test_misaligned_base_is_refused():
    """A base off by one word at D % 4 == 0: refused (amdspeech.h), in both modes and by the moments; the tensor is not written.
    At D % 4 != 0 the same base runs."""
    from rnn_speech_amd import lib, ops
    t_in, B, D = 6, 2, 8
    flat = torch.arange(t_in * B * D + 1, dtype=torch.float32).cuda()
    x = flat[1:].view(t_in, B, D)
    assert x.is_contiguous() and x.data_ptr() % 16 == 4
    before = bits(x).copy()
    table = torch.ones(2, D, dtype=torch.float64).cuda()
    for call in (lambda: ops.feature_norm(x, [6, 4], "utterance"), lambda: ops.feature_norm(x, [6, 4], "global", table=table),
                 lambda: ops.feature_moments(x, [6, 4])):
        with pytest.raises(lib.AmdSpeechError, match="16-byte aligned"):
            call()
    torch.cuda.synchronize()
    assert np.array_equal(bits(x), before)
    odd = flat[1:1 + 6 * 2 * 7].view(6, 2, 7)
    want = odd.cpu().numpy().copy()
    got = ops.feature_norm(odd, [6, 4], "utterance").cpu().numpy()
    assert ref.passes(ref.judge(got, want, [6, 4]))


# ------------------------------------------------------------------------------------------------ 2. global mode
@pytest.mark.parametrize("name", ["vec4_d40", "vec4_d120", "vec1_d13", "wide_batch", "widest_frame", "vec1_columns", "row_stride"])
def test_global_mode_is_bit_identical_to_numpy(name):
    """float32((float64(x) - mean) * scale) on the valid frames, nothing else written: uint32 equality, no tolerance."""
    from rnn_speech_amd import ops
    D, t_in, B, _, _ = ref.CASES[name]
    x, lengths = ref.case_inputs(name)
    rng = np.random.RandomState(D + B)
    table = np.stack([rng.uniform(-1200, 1200, size=D), 10.0 ** rng.uniform(-3, 2, size=D)])
    plan = ops.feature_norm_plan(B, D, t_in, "global")
    assert plan == ref.expected_plan(B, D, t_in, "global") and plan["workspace_bytes"] == 0
    got = ops.feature_norm(upload(x), [int(n) for n in lengths], "global", table=upload(table))
    assert np.array_equal(bits(got), ref.normalise_global(x, lengths, table).view(np.uint32))
    with pytest.raises(ValueError):
        ops.feature_norm(upload(x), [int(n) for n in lengths], "global")                        # no table
    with pytest.raises(ValueError):
        ops.feature_norm(upload(x), [int(n) for n in lengths], "global", table=upload(table.astype(np.float32)))
    with pytest.raises(ValueError):
        ops.feature_norm(upload(x), [int(n) for n in lengths], "utterance", table=upload(table))


# ------------------------------------------------------------------------------------------------ 3. moments and corpus statistics
def _moments_within_bounds(got, x, lengths):
    """mean to 1e-13 of max|x|, M2 to 1e-10 relative (both float64 quantities; empty rows: zeros).

    Derivation.  S' and Q' are float64 sums of the shifted frames; an addition loses at most 2^-53 of the running sum, so a chain
    of m terms loses at most m 2^-53 of sum |term|.  A row has n <= 2^20 frames, spread over split x slots chains that are then
    added in order, so m <= n / (split slots) + slots + split <= n: at most 2^20 2^-53 = 1.2e-10 for one chain of the longest row
    the front end can emit, and m <= 1001 -> 1.1e-13 for every row here.  mean = K + S'/n adds |K| 2^-53: within 1e-13 max|x|.
    M2 = Q' - S'^2 / n cancels when the shift K is far from the mean: the relative loss grows by 1 + (mean - K)^2 / var, below 20
    with K the row's first frame within four deviations of its mean -- 1001 2^-53 20 = 2.2e-12, under 1e-10 with room."""
    want = ref.moments(x, lengths)
    top = max(float(np.abs(x[:n, b].astype(np.float64)).max()) for b, n in enumerate(ref.clipped(lengths, x.shape[0])) if n > 0)
    assert got.shape == want.shape and got.dtype == np.float64
    assert np.all(np.abs(got[:, 0] - want[:, 0]) <= 1e-13 * top), np.abs(got[:, 0] - want[:, 0]).max() / top
    assert np.all(np.abs(got[:, 1] - want[:, 1]) <= 1e-10 * want[:, 1]), (np.abs(got[:, 1] - want[:, 1]) / np.maximum(want[:, 1], 1e-300)).max()
    for b, n in enumerate(lengths):
        if n == 0:
            assert not got[b].any()


@pytest.mark.parametrize("name", ["offset_split", "vec4_d120", "vec1_d13", "wide_batch", "tiny_variance", "vec1_columns"])
def test_moments_against_float64(name):
    from rnn_speech_amd import ops
    x, lengths = ref.case_inputs(name)
    dx = upload(x)
    got = ops.feature_moments(dx, [int(n) for n in lengths])
    assert got.dtype == torch.float64 and got.is_cuda
    _moments_within_bounds(got.cpu().numpy(), x, lengths)
    assert np.array_equal(bits(dx), x.view(np.uint32))                  # the features are not written
    again = ops.feature_moments(dx, [int(n) for n in lengths])
    assert torch.equal(again, got)


def test_feature_stats_over_two_mini_batches():
    from rnn_speech_amd.feature_norm import FeatureStats, describe
    batches = [ref.case_inputs("offset_split"), ref.case_inputs("vec4_d40")]
    frames = np.concatenate([x[:n, b] for x, lengths in batches for b, n in enumerate(ref.clipped(lengths, x.shape[0]))]).astype(np.float64)
    stats = FeatureStats(describe("mfcc", 40, 16000, 40))
    for x, lengths in batches:
        stats.accumulate(upload(x), [int(n) for n in lengths])
    assert stats.count == len(frames) == 1001 + 1001 + 700 + 0 + 1 + 2 + 70 + 70
    mean = frames.sum(axis=0) / len(frames)
    m2 = ((frames - mean) ** 2).sum(axis=0)
    assert np.all(np.abs(stats.mean - mean) <= 1e-13 * np.abs(frames).max())
    assert np.all(np.abs(stats.M2 - m2) <= 1e-10 * m2)
    table = stats.table()
    assert table.is_cuda and table.dtype == torch.float64 and np.array_equal(table.cpu().numpy(), stats.table_numpy())


# ------------------------------------------------------------------------------------------------ 4. through the front end
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
    feat, n = plain.process_batch(signals, sr)
    src = feat.cpu().numpy().copy()
    assert max(n) > T > min(n) and not src[min(n):, 0].any()
    utt = AudioProcessor(T, "mfcc", n_mfcc=40, load_sr=sr, feature_norm="utterance")
    got, got_n = utt.process_batch(signals, sr)
    assert list(got_n) == list(n) and got.shape == feat.shape
    verdict = ref.judge(got.cpu().numpy(), src, n)                       # (the front end's zeros past each length are still zeros)
    assert ref.passes(verdict), verdict
    c0_before, c0_after = float(src[:26, 0, 0].astype(np.float64).mean()), float(got[:26, 0, 0].double().mean())
    print("FEATNORM front_end c0_mean_before=%.4g after=%.3g" % (c0_before, c0_after))
    assert abs(c0_after) < 1e-5 and abs(c0_before) > 1e4 * abs(c0_after)                            # c0 was not zero-mean; it is now

    # low frame rate input behind it stacks the NORMALISED frames
    lfr = AudioProcessor(T, "mfcc", n_mfcc=40, load_sr=sr, feature_norm="utterance", frame_stack=3, frame_skip=3)
    stacked, stacked_n = lfr.process_batch(signals, sr)
    want, want_n = frame_stack_ref.stack(bits(got), n, 3, 3)
    assert stacked.shape == (20, 3, 120) and np.array_equal(bits(stacked), want) and list(stacked_n) == list(want_n)

    # means only, and the reference surface of one signal (its own batch of one: another plan, the same bound)
    only_mean, _ = AudioProcessor(T, "mfcc", n_mfcc=40, load_sr=sr, feature_norm="utterance", feature_norm_variance=False).process_batch(signals, sr)
    assert ref.passes(ref.judge(only_mean.cpu().numpy(), src, n, norm_vars=False))
    one, one_n = utt.process_signal(signals[2], sr)
    src_one, src_n = plain.process_signal(signals[2], sr)
    assert one_n == src_n == n[2] and one.shape == (T, 40)
    assert ref.passes(ref.judge(one[:, None, :], src_one[:, None, :], [src_n]))

    # global mode reads the table of its statistics: bit for bit the numpy formula
    from rnn_speech_amd.feature_norm import FeatureStats, describe_processor
    stats = FeatureStats(describe_processor(plain)).accumulate(feat, n)
    assert stats.count == 26 + 46 + 60
    glob = AudioProcessor(T, "mfcc", n_mfcc=40, load_sr=sr, feature_norm="global", feature_stats=stats)
    gg, _ = glob.process_batch(signals, sr)
    assert np.array_equal(bits(gg), ref.normalise_global(src, n, stats.table_numpy()).view(np.uint32))

    # none: the front end's own tensor -- nothing is copied, nothing is launched
    seen, calls = {}, []
    real, real_norm = ops.frontend, ops.feature_norm

    def spy(*a, **kw):
        seen["feat"], seen["n"] = real(*a, **kw)
        return seen["feat"], seen["n"]

    ops.frontend, ops.feature_norm = spy, lambda *a, **kw: calls.append(a) or real_norm(*a, **kw)
    try:
        same, same_n = plain.process_batch(signals, sr)
        assert same is seen["feat"] and same_n is seen["n"] and not calls
        utt.process_batch(signals, sr)
        assert len(calls) == 1 and calls[0][0] is seen["feat"]           # ... and utterance mode normalises that tensor in place
    finally:
        ops.frontend, ops.feature_norm = real, real_norm


# ------------------------------------------------------------------------------------------------ 5. through the model
def test_through_the_model():
    """Engine(2, 128, 120, 80, 20, 10, 3) on ops.feature_norm of a [10, 20, 120] input with a large offset per dim against
    oracle.model on the float64-normalised input.  Tolerances: tests/test_gpu_model.py::test_forward_backward_adam_parity's,
    unchanged."""
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
    src = (rng.uniform(-1200, 1200, size=D) + 10.0 ** rng.uniform(-1, 1.5, size=D) * rng.randn(T, B, D)).astype(np.float32)
    lengths = rng.randint(7, 11, size=B).astype(np.int32)
    dense = np.zeros((B, U), np.int32)
    for b in range(B):
        n = rng.randint(1, U)
        dense[b, :n] = rng.randint(1, C - 1, size=n)
        dense[b, n] = C - 1
    x64 = ref.normalise(src, lengths)
    for b, n in enumerate(lengths):
        x64[n:, b] = 0.0                        # (the model never reads them; the oracle wants finite numbers there)
        src[n:, b] = 0.0
    assert lengths.min() >= 2 * U + 1 == 7 and lengths.max() <= T and np.abs(x64).max() < 4

    dx = ops.feature_norm(upload(src), [int(v) for v in lengths], "utterance")
    assert ref.passes(ref.judge(dx.cpu().numpy(), src, lengths))

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


# ------------------------------------------------------------------------------------------------ 6. drop-in
TEXTS = ["hello there", "it'll do"]


def _write_wav(path, seed, seconds, sr=22050):
    rng = np.random.RandomState(seed)
    t = np.arange(int(seconds * sr)) / float(sr)
    sig = 0.05 * rng.randn(len(t)) + 0.3 * np.sin(2 * np.pi * (200 + 50 * seed) * t)
    with wave.open(path, "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(sr)
        w.writeframes((np.clip(sig, -1, 1) * 32767).astype("<i2").tobytes())


def _config(tmp_path, mode, n_mfcc=20):
    """config.ini with feature_norm : mode -> the hyper parameters the way stt.py reads them, and two short recordings."""
    from models.SpeechRecognizer import SpeechRecognizer
    from util.hyperparams import read_config_file
    src = open(os.path.join(ROOT, "config.ini")).read()
    src = src.replace("checkpoint_dir", "checkpoint_dir : %s\n#" % (tmp_path / ("ckpt_" + mode)), 1)
    for old, new in (("feature_norm : none", "feature_norm : " + mode),
                     ("feature_norm_stats : data/feature_stats.npz", "feature_norm_stats : %s" % (tmp_path / "stats" / "train.npz")),
                     ("max_input_seq_length : 1001", "max_input_seq_length : 90"), ("max_target_seq_length : 161", "max_target_seq_length : 12"),
                     ("num_layers : 3", "num_layers : 2"), ("hidden_size : 512", "hidden_size : 64"), ("batch_size : 32", "batch_size : 2"),
                     ("n_mfcc : 40", "n_mfcc : %d" % n_mfcc), ("feature_cache_mb : 0", "feature_cache_mb : 4"), ("train_decoder : beam", "train_decoder : greedy")):
        assert old in src
        src = src.replace(old, new, 1)
    cfg = tmp_path / ("config_%s.ini" % mode)
    cfg.write_text(src)
    hp = read_config_file(str(cfg))
    reco = SpeechRecognizer(hp["language"])
    hp["char_map"], hp["char_map_length"] = reco.get_char_map(), reco.get_char_map_length()
    items = []
    for i, (txt, seconds) in enumerate(zip(TEXTS, (0.6, 1.2))):         # 61 and 121 source frames: the second is truncated at 90
        path = str(tmp_path / ("u%d.wav" % i))
        if not os.path.exists(path):
            _write_wav(path, i, seconds)
        items.append([path, txt, None])
    return hp, items


def _one_step(stt, hp, items, want_of):
    """The model, the iterators and one training step the way stt.py runs them; the batch and the feature cache against
    want_of(plain features, lengths)."""
    from models.AcousticModel import Session
    stt.build_audio_processor(hp)
    sess = Session()
    model, t_it, v_it = stt.build_acoustic_training_rnn(sess, hp, dict(tb_name=None, timeline=False, learn_rate=None), items, items[:1])
    try:
        eng, train = model.engine, t_it.dataset
        assert (eng.D, eng.T, eng.B) == (20, 90, 2)
        assert (model.feature_norm, train.audio.feature_norm, v_it.dataset.audio.feature_norm) == (hp["feature_norm"],) * 3
        loss, err, step, exhausted = model.run_train_step(sess, 1, 1.0)
        assert step == 1 and np.isfinite(loss)
        eng.check()
        plain = stt.AcousticModel.build_dataset(items, 2, 90, 12, "mfcc", hp["char_map"], n_mfcc=20)
        (fp, np_, _), = list(plain.batches())
        assert list(np_) == [61, 121]
        # the same batch a second time comes out of the feature cache and is the same batch, bit for bit
        assert set(train._cache) == {items[0][0], items[1][0]}
        fresh = stt.AcousticModel.build_dataset(items, 2, 90, 12, "mfcc", hp["char_map"], n_mfcc=20, feature_norm=hp["feature_norm"],
                                                feature_stats=train.audio.feature_stats)
        (f0, n0, d0), = list(fresh.batches())
        (f1, n1, d1), = list(train.with_items(items).batches())
        assert f0.shape == (90, 2, 20) and list(n0) == list(n1) == [61, 121] and np.array_equal(d0, d1)
        assert np.array_equal(bits(f0), bits(f1))
        want_of(f0.cpu().numpy(), fp.cpu().numpy(), np_)
        assert not f0[61:, 0].any()                      # past the utterance: the front end's zeros
    finally:
        model.close()


def test_drop_in_global_from_config(tmp_path):
    """--feature_stats over two recordings writes the statistics numpy takes over the plain features; `feature_norm : global` then
    reaches the processor, the datasets and the engine; one train step; the feature cache; a file of other features is refused."""
    import stt
    from rnn_speech_amd.feature_norm import FeatureStats
    from util.audioprocessor import AudioProcessor
    hp, items = _config(tmp_path, "global")
    path = hp["feature_norm_stats"]
    assert hp["feature_norm"] == "global" and not os.path.exists(path)
    stats = stt.feature_stats(items, hp)                 # (normalisation off whatever the config says: the file does not exist yet)
    plain = stt.AcousticModel.build_dataset(items, 2, 90, 12, "mfcc", hp["char_map"], n_mfcc=20)
    (fp, np_, _), = list(plain.batches())
    fp = fp.cpu().numpy()
    frames = np.concatenate([fp[:61, 0], fp[:90, 1]]).astype(np.float64)
    mean = frames.sum(axis=0) / len(frames)
    var = ((frames - mean) ** 2).sum(axis=0) / len(frames)
    with np.load(path) as z:
        assert float(z["count"]) == stats.count == 151 and int(z["n_mfcc"]) == 20 and int(z["width"]) == 20 and int(z["sample_rate"]) == 22050
        assert str(z["signal_processing"]) == "mfcc"
        assert np.all(np.abs(z["mean"] - mean) <= 1e-13 * np.abs(frames).max())
        assert np.all(np.abs(z["var"] - var) <= 1e-10 * var)
    table = FeatureStats.load(path).table_numpy()

    def want_of(got, plain_feat, lengths):
        assert np.array_equal(got.view(np.uint32), ref.normalise_global(plain_feat, lengths, table).view(np.uint32))

    _one_step(stt, hp, items, want_of)
    with pytest.raises(ValueError, match="the processor computes"):       # statistics of 20 coefficients, a processor of 40
        AudioProcessor(90, "mfcc", n_mfcc=40, feature_norm="global", feature_stats=path)
    hp40, _ = _config(tmp_path, "global", n_mfcc=40)
    with pytest.raises(ValueError, match="the processor computes"):
        stt.build_audio_processor(hp40)


def test_drop_in_utterance_from_config(tmp_path):
    import stt
    hp, items = _config(tmp_path, "utterance")
    assert hp["feature_norm"] == "utterance"

    def want_of(got, plain_feat, lengths):
        verdict = ref.judge(got, plain_feat, lengths)
        assert ref.passes(verdict), verdict

    _one_step(stt, hp, items, want_of)
    assert not os.path.exists(hp["feature_norm_stats"])  # the statistics file belongs to global mode only
