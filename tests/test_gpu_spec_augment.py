"""SpecAugment on the GPU (csrc/spec_augment.hip): the kernel bit for bit against tests/spec_augment_ref.py at the edges, its
determinism, the off policies, through the model against the float64 oracle, and as a config.ini drop-in the way stt.py builds it."""
import os
import sys
import wave

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import model as om  # noqa: E402  (checker only)

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import spec_augment_ref as ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bits(t):
    return t.cpu().numpy().view(np.uint32)


def upload(x):
    return torch.from_numpy(x.view(np.float32).copy()).cuda()          # (the shared arrays are read-only)


def upload_lengths(lengths):
    return torch.from_numpy(lengths.copy()).cuda()


_WANT = {}


def case(name):
    """(x, lengths, policy, expected) of a case; the reference runs once per case and is shared, unchanged, by the tests."""
    if name not in _WANT:
        x, lengths = ref.case_inputs(name)
        pol = ref.case_policy(name)
        want = ref.apply(x, lengths, pol, ref.SEED)
        for a in (x, lengths, want):
            a.setflags(write=False)
        _WANT[name] = (x, lengths, pol, want)
    return _WANT[name]


# ------------------------------------------------------------------------------------------------ 1. bit-exact at the edges
@pytest.mark.parametrize("name", sorted(ref.CASES))
def test_bit_exact_at_the_edges(name):
    """uint32 bit patterns, np.array_equal: masked words are exactly 0x00000000 and every other word -- -0.0, a denormal, +-inf and
    a NaN payload in the live region, the poison at every frame at or past a row's length -- is unchanged.  So are the lengths."""
    from rnn_speech_amd import ops
    T, B, W = ref.CASES[name][:3]
    x, lengths, pol, want = case(name)
    plan = ops.spec_augment_plan(T, B, W, pol)
    assert plan == ref.expected_plan(T, B, W, pol) and plan["workgroups"] > 0
    if name == "stride":
        assert plan["workgroups"] == ref.MAX_WGS and T * B > ref.MAX_WGS * plan["items_per_workgroup"]      # the grid strides
    dx, dlen = upload(x), upload_lengths(lengths)
    assert dx.data_ptr() % 16 == 0 and np.array_equal(bits(dx), x)         # the upload keeps the patterns
    got = ops.spec_augment(dx, dlen, pol, ref.SEED)
    torch.cuda.synchronize()
    assert got is dx
    g = bits(dx)
    changed = g != x
    assert np.all(g[changed] == 0), "a word was changed to something other than +0.0"
    assert np.array_equal(g == ref.POISON, x == ref.POISON), "a frame at or past its row's length was written"
    assert np.array_equal(g, want)
    assert changed.any() and np.array_equal(dlen.cpu().numpy(), lengths)


@pytest.mark.parametrize("name", ["vec4_p40", "stacked_p13x4", "cap_zero"])
def test_a_base_that_is_not_16_byte_aligned_takes_single_word_stores(name):
    """W % 4 == 0 on a tensor that starts one word into its allocation: the call plans with vec = 1 and the result is the same."""
    from rnn_speech_amd import ops
    T, B, W = ref.CASES[name][:3]
    x, lengths, pol, want = case(name)
    guard = np.uint32(0xCDCDCDCD)
    buf = torch.from_numpy(np.concatenate([[guard], x.reshape(-1), [guard]]).view(np.float32)).cuda()
    dx = buf[1:-1].view(T, B, W)
    assert dx.is_contiguous() and dx.data_ptr() % 16 == 4
    ops.spec_augment(dx, upload_lengths(lengths), pol, ref.SEED)
    torch.cuda.synchronize()
    assert np.array_equal(bits(dx), want)
    assert bits(buf)[0] == guard and bits(buf)[-1] == guard


# ------------------------------------------------------------------------------------------------ 2. seeds
def test_same_seed_same_masks_other_seed_other_masks():
    from rnn_speech_amd import ops
    x, lengths, pol, want = case("fbank_p40x3")
    dlen = upload_lengths(lengths)
    a, b, c = upload(x), upload(x), upload(x)
    ops.spec_augment(a, dlen, pol, ref.SEED)
    ops.spec_augment(b, dlen, pol, ref.SEED)
    assert np.array_equal(bits(a), bits(b)) and np.array_equal(bits(a), want)
    ops.spec_augment(b, dlen, pol, ref.SEED)                  # a second time on the result: nothing changes
    assert np.array_equal(bits(b), want)
    other = ref.SEED + 1
    ops.spec_augment(c, dlen, pol, other)
    assert np.array_equal(bits(c), ref.apply(x, lengths, pol, other))
    assert not np.array_equal(bits(c) == 0, want == 0)


# ------------------------------------------------------------------------------------------------ 3. off
def test_off_means_nothing_launched():
    from rnn_speech_amd import lib, ops
    x, lengths, pol, want = case("vec4_p40")
    dlen = upload_lengths(lengths)
    handle = lib.load()
    real = handle.amdspeech_spec_augment
    calls = []

    def spy(*args):
        calls.append(args)
        return real(*args)

    handle.amdspeech_spec_augment = spy
    try:
        for off in (ref.policy(40, 0, 0, 0, 0, 1000), ref.policy(40, 0, 7, 0, 5, 1000), ref.policy(40, 2, 0, 2, 0, 1000)):
            assert ops.spec_augment_plan(x.shape[0], x.shape[1], x.shape[2], off)["workgroups"] == 0
            dx = upload(x)
            assert ops.spec_augment(dx, dlen, off, ref.SEED) is dx
            torch.cuda.synchronize()
            assert np.array_equal(bits(dx), x)
        assert calls == []
        dx = upload(x)                                        # (the spy does see a launch)
        ops.spec_augment(dx, dlen, pol, ref.SEED)
        assert len(calls) == 1 and np.array_equal(bits(dx), want)
    finally:
        handle.amdspeech_spec_augment = real
    with pytest.raises(ValueError):
        ops.spec_augment(upload(x).transpose(0, 1), dlen, pol, ref.SEED)             # not contiguous
    with pytest.raises(ValueError):
        ops.spec_augment(upload(x).double(), dlen, pol, ref.SEED)
    with pytest.raises(ValueError):
        ops.spec_augment(upload(x)[0], dlen, pol, ref.SEED)                          # two dimensions
    with pytest.raises(ValueError):
        ops.spec_augment(upload(x), torch.from_numpy(lengths.copy()), pol, ref.SEED)        # lengths on the host
    with pytest.raises(ValueError):
        ops.spec_augment(upload(x), dlen.long(), pol, ref.SEED)
    with pytest.raises(ValueError):
        ops.spec_augment(upload(x), dlen[:-1], pol, ref.SEED)


# ------------------------------------------------------------------------------------------------ 4. through the model
def test_through_the_model():
    """Engine(2, 128, 120, 80, 20, 10, 3) on ops.spec_augment of a random [10, 20, 120] input with P = 40 against oracle.model on
    the numpy-masked float64 input.  Tolerances: tests/test_gpu_frame_stack.py::test_through_the_model's, unchanged.  dW_i is the
    only gradient that reads the masked words."""
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
    src = rng.randn(T, B, D).astype(np.float32)
    lengths = rng.randint(7, T + 1, size=B).astype(np.int32)
    dense = np.zeros((B, U), np.int32)
    for b in range(B):
        n = rng.randint(1, U)
        dense[b, :n] = rng.randint(1, C - 1, size=n)
        dense[b, n] = C - 1
    assert lengths.min() >= 2 * U + 1 == 7 and lengths.max() <= T          # every row has a feasible alignment
    pol = ref.policy(40, 2, 8, 2, 3, 1000)
    x64 = ref.apply(src.astype(np.float64), lengths, pol, ref.SEED)
    masked = (x64 == 0) & (src != 0)
    assert masked.any() and not masked.all() and masked.sum() > 1000

    dx, dlen = torch.as_tensor(src).cuda(), torch.as_tensor(lengths).cuda()
    ops.spec_augment(dx, dlen, pol, ref.SEED)
    assert np.array_equal(dx.cpu().numpy(), x64.astype(np.float32))

    p64 = {key: v.astype(np.float64) for key, v in p.items()}
    logits_ref, _, cache = om.forward(p64, x64, lengths, L, keep_cache=True)
    loss_ref, dl_ref = om.ctc_loss_and_grad(logits_ref, om.sparsify_labels(dense, C), lengths)
    g_ref = om.backward(p64, cache, dl_ref, lengths, L)
    assert np.all(np.isfinite(loss_ref)) and np.all(loss_ref > 0)

    eng.zero_grads()
    eng.mini_batch(dx, dlen, torch.as_tensor(dense).cuda())
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


# ------------------------------------------------------------------------------------------------ 5. drop-in
def _write_wav(path, seed, seconds, sr=22050):
    rng = np.random.RandomState(seed)
    t = np.arange(int(seconds * sr)) / float(sr)
    sig = 0.05 * rng.randn(len(t)) + 0.3 * np.sin(2 * np.pi * (200 + 50 * seed) * t)
    with wave.open(path, "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(sr)
        w.writeframes((np.clip(sig, -1, 1) * 32767).astype("<i2").tobytes())


CONFIG_SEED = 5
TEXTS = ["hello there", "it'll do"]


def _build(tmp_path, frame_stack):
    """config.ini with the spec_augment_* keys on -> the model, the iterators and the items the way stt.py builds them."""
    import stt
    from models.AcousticModel import Session
    from models.SpeechRecognizer import SpeechRecognizer
    from util.hyperparams import read_config_file
    src = open(os.path.join(ROOT, "config.ini")).read()
    src = src.replace("checkpoint_dir", "checkpoint_dir : %s\n#" % (tmp_path / "ckpt"), 1)
    for old, new in (("frame_stack : 1", "frame_stack : %d" % frame_stack), ("frame_skip : 1", "frame_skip : %d" % frame_stack),
                     ("max_input_seq_length : 1001", "max_input_seq_length : 90"), ("max_target_seq_length : 161", "max_target_seq_length : 12"),
                     ("num_layers : 3", "num_layers : 2"), ("hidden_size : 512", "hidden_size : 64"), ("batch_size : 32", "batch_size : 2"),
                     ("n_mfcc : 40", "n_mfcc : 20"), ("feature_cache_mb : 0", "feature_cache_mb : 4"), ("train_decoder : beam", "train_decoder : greedy"),
                     ("spec_augment_freq_masks : 0", "spec_augment_freq_masks : 2"), ("spec_augment_freq_width : 0", "spec_augment_freq_width : 6"),
                     ("spec_augment_time_masks : 0", "spec_augment_time_masks : 2"), ("spec_augment_time_width : 0", "spec_augment_time_width : 8"),
                     ("spec_augment_time_ratio : 1.0", "spec_augment_time_ratio : 0.5"), ("spec_augment_seed : 0", "spec_augment_seed : %d" % CONFIG_SEED)):
        assert old in src
        src = src.replace(old, new, 1)
    cfg = tmp_path / "config.ini"
    cfg.write_text(src)
    hp = read_config_file(str(cfg))
    stt.build_audio_processor(hp)
    reco = SpeechRecognizer(hp["language"])
    hp["char_map"], hp["char_map_length"] = reco.get_char_map(), reco.get_char_map_length()
    pol = dict(period=20, freq_masks=2, freq_width=6, time_masks=2, time_width=8, time_permille=500, seed=CONFIG_SEED)
    assert hp["spec_augment"] == pol and hp["input_dim"] == 20 * frame_stack          # the period is the SOURCE frame's width
    items = []
    for i, (txt, seconds) in enumerate(zip(TEXTS, (0.6, 1.2))):         # 61 and 121 source frames: the second is truncated at 90
        path = str(tmp_path / ("u%d.wav" % i))
        _write_wav(path, i, seconds)
        items.append([path, txt, None])
    sess = Session()
    model, t_it, v_it = stt.build_acoustic_training_rnn(sess, hp, dict(tb_name=None, timeline=False, learn_rate=None), items, items[:1])
    assert model.spec_augment == pol
    return stt, hp, sess, model, t_it, v_it, items, pol


def _step_seed(counter, rank=0):
    """The seed rule of AcousticModel.run_step, restated."""
    return ((CONFIG_SEED + rank) << 32) | ((counter * 0x9E3779B1) & 0xFFFFFFFF)


class _Spy(object):
    """Records what reaches a bound method of the engine (a copy of the first argument's bits and its address)."""

    def __init__(self, owner, name):
        self.owner, self.name, self.real, self.seen = owner, name, getattr(owner, name), []
        setattr(owner, name, self)

    def __call__(self, x, *args, **kwargs):
        self.seen.append((bits(x).copy(), x.data_ptr(), kwargs))
        return self.real(x, *args, **kwargs)

    def undo(self):
        delattr(self.owner, self.name)


def test_drop_in_from_config(tmp_path):
    """The keys reach the model the way stt.py builds it; a training step masks what the engine reads -- from the front end, from
    the feature cache and from feed() -- under the seed rule, and nothing a caller can reach; evaluation and process_input never
    mask."""
    stt, hp, sess, model, t_it, v_it, items, pol = _build(tmp_path, 1)
    try:
        eng, train = model.engine, t_it.dataset
        T = eng.T
        assert (eng.D, T, eng.B) == (20, 90, 2)
        plain = stt.AcousticModel.build_dataset(items, 2, 90, 12, "mfcc", hp["char_map"], n_mfcc=20)
        (f0, n0, d0), = list(plain.batches())
        x0 = bits(f0).copy()
        assert list(n0) == [61, 121]
        spy = _Spy(eng, "mini_batch")

        # 1. the iterator's batch, straight from the front end
        loss, err, step, exhausted = model.run_train_step(sess, 1, 1.0)
        assert step == 1 and np.isfinite(loss) and model._dropout_seed == 1
        eng.check()
        want1 = ref.apply(x0, n0, pol, _step_seed(1))
        assert len(spy.seen) == 1 and np.array_equal(spy.seen[0][0], want1)
        assert (want1 != x0).any() and (want1 == x0)[:61, 0].sum() > 10
        cache = {k: (f.copy(), n) for k, (f, n) in train._cache.items()}
        assert set(cache) == {items[0][0], items[1][0]}
        for row, (path, _, _) in enumerate(items):                       # the cache holds the UNmasked features
            f, n = cache[path]
            assert n == n0[row] and np.array_equal(f.view(np.uint32), x0[:min(n, T), row])

        # 2. the next epoch comes out of the feature cache: another seed, the cache as it was
        sess.run(t_it.make_initializer(train.with_items(items)))
        loss, err, step, exhausted = model.run_train_step(sess, 1, 1.0)
        assert step == 2 and np.isfinite(loss) and model._dropout_seed == 2
        want2 = ref.apply(x0, n0, pol, _step_seed(2))
        assert len(spy.seen) == 2 and np.array_equal(spy.seen[1][0], want2) and not np.array_equal(want1 == 0, want2 == 0)
        assert set(train._cache) == set(cache)
        for path, (f, n) in cache.items():
            assert train._cache[path][1] == n and np.array_equal(train._cache[path][0].view(np.uint32), f.view(np.uint32))

        # 3. a batch a caller holds -- out of dataset.batches(), handed in through feed() as a device tensor -- is not written
        (fb, nb, db), = list(train.with_items(items).batches())
        assert fb.is_cuda and fb.is_contiguous() and np.array_equal(bits(fb), x0)
        model.feed(fb, nb, db)
        loss, err, step, exhausted = model.run_train_step(sess, 1, 1.0)
        torch.cuda.synchronize()
        assert step == 3 and np.isfinite(loss)
        eng.check()
        assert len(spy.seen) == 3 and np.array_equal(spy.seen[2][0], ref.apply(x0, n0, pol, _step_seed(3)))
        assert spy.seen[2][1] != fb.data_ptr() and np.array_equal(bits(fb), x0)
        # ... and a host array through feed() is masked on its device copy
        host = f0.cpu().numpy()
        model.feed(host, nb, db)
        model.run_train_step(sess, 1, 1.0)
        assert np.array_equal(spy.seen[3][0], ref.apply(x0, n0, pol, _step_seed(4))) and np.array_equal(host.view(np.uint32), x0)

        # 4. evaluation never masks
        (fv, nv, dv), = list(v_it.dataset.with_items(items[:1]).batches())
        model.run_evaluation(sess)
        assert len(spy.seen) == 5 and spy.seen[4][2]["compute_gradients"] is False
        assert np.array_equal(spy.seen[4][0], bits(fv)) and np.array_equal(bits(fv)[:, 0], x0[:, 0])
        spy.undo()

        # 5. ... nor does process_input
        fwd = _Spy(eng, "forward")
        model.process_input(sess, fb, np.minimum(nb, T))
        fwd.undo()
        assert len(fwd.seen) == 1 and np.array_equal(fwd.seen[0][0], x0) and np.array_equal(bits(fb), x0)
    finally:
        model.close()


def test_drop_in_under_frame_stack(tmp_path):
    """frame_stack : 3 / frame_skip : 3: the model frame is 60 wide, the period stays the source frame's 20, and a masked bin is
    zero in all three stacked sub-frames."""
    from rnn_speech_amd import ops
    stt, hp, sess, model, t_it, v_it, items, pol = _build(tmp_path, 3)
    try:
        eng = model.engine
        T = eng.T
        assert (eng.D, T, eng.B) == (60, 30, 2) and pol["period"] == 20
        plain = stt.AcousticModel.build_dataset(items, 2, 90, 12, "mfcc", hp["char_map"], n_mfcc=20, frame_stack=3, frame_skip=3)
        (f0, n0, d0), = list(plain.batches())
        x0 = bits(f0).copy()
        assert list(n0) == [21, 41]
        spy = _Spy(eng, "mini_batch")
        loss, err, step, exhausted = model.run_train_step(sess, 1, 1.0)
        spy.undo()
        assert step == 1 and np.isfinite(loss)
        eng.check()
        got = spy.seen[0][0]
        assert np.array_equal(got, ref.apply(x0, n0, pol, _step_seed(1)))
        bins = 0
        for b in range(2):
            n = min(int(n0[b]), T)
            spans = ops.spec_augment_spans(pol, _step_seed(1), b, n)
            assert spans == ref.spans(pol, _step_seed(1), b, n)
            for start, width in spans[:2]:
                for k in range(start, start + width):
                    bins += 1
                    assert all(np.all(got[:n, b, i * 20 + k] == 0) for i in range(3)), (b, k)
        assert bins > 0
    finally:
        model.close()
