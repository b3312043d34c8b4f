"""Blank-frame skipping on the GPU (csrc/ctc_blank_skip.hip) against tests/blank_skip_ref.py: every case of the table through the C
ABI -- blank_logp within the derived bound of float64, out_lengths, src_frame and out_logits bit for bit, tail words included --,
two calls the same bits, a row's outputs independent of its place in the batch, both row kernels named by the plan, what the call
refuses, and the key decode_blank_skip in a small model: off it changes nothing and launches nothing, on it the beam decoders
return the same strings from fewer frames.

The table (blank_skip_ref.cases): every C of {2, 5, 80, 81} and on either side of each c_min / c_max boundary of the plan at T 7, B 3;
every T of {1, 2, 3, chunk - 1, chunk, chunk + 1, 2 chunk + 1} at C 5 (single words) and C 80 (16-byte vectors); B of {1, 3, 33};
every frame pattern at T = 2 chunk + 1 and at T = 9; lengths of 0, 1, T, T + 5 and a negative one cycle over the rows."""
import ctypes

import numpy as np
import pytest
import torch

import blank_skip_ref as R
from rnn_speech_amd import lib, ops

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def table():
    """(case, reference) pairs: the references are computed once and shared, read-only."""
    return [(c, R.blank_skip_ref(c["logits"], c["lengths"], c["theta"])) for c in R.cases(ops.ctc_blank_skip_plan)]


def _run(logits, lengths, theta, poison=True):
    """One call into poisoned outputs (whatever was there must be overwritten): host copies as blank_skip_ref names them."""
    T, B, C = logits.shape
    x = torch.from_numpy(np.ascontiguousarray(logits)).cuda()
    n = torch.from_numpy(np.asarray(lengths, np.int32)).cuda()
    out = torch.full((T, B, C), 7.0, device="cuda") if poison else None
    new_len = torch.full((B,), -9, device="cuda", dtype=torch.int32)
    src = torch.full((B, T), 12345, device="cuda", dtype=torch.int32)
    lpb = torch.full((T, B), 7.0, device="cuda")
    out, new_len, src = ops.ctc_blank_skip(x, n, theta, out=out, new_lengths=new_len, src_frame=src, blank_logp=lpb)
    return dict(out_logits=out.cpu().numpy(), out_lengths=new_len.cpu().numpy(), src_frame=src.cpu().numpy(), blank_logp=lpb.cpu().numpy())


def test_every_case_against_the_reference_and_twice_the_same_bits(table):
    worst = 0.0
    for c, ref in table:
        got = _run(c["logits"], c["lengths"], c["theta"])
        with np.errstate(invalid="ignore"):
            M = np.nanmax(np.abs(c["logits"].astype(np.float64)), axis=2)
        bound = R.lpb_bound(c["C"], M)
        err = np.abs(got["blank_logp"].astype(np.float64) - ref["blank_logp"])
        assert np.array_equal(np.isnan(err), np.isnan(ref["blank_logp"])), c["name"]
        ratio = float(np.nanmax(err / bound))
        print("%s: |lpb - float64| / bound %.3g" % (c["name"], ratio))
        assert ratio <= 1.0, c["name"]
        worst = max(worst, ratio)
        assert np.array_equal(got["out_lengths"], ref["out_lengths"]), (c["name"], got["out_lengths"], ref["out_lengths"])
        assert np.array_equal(got["src_frame"], ref["src_frame"]), c["name"]
        assert got["out_logits"].tobytes() == ref["out_logits"].tobytes(), c["name"]
        again = _run(c["logits"], c["lengths"], c["theta"], poison=False)
        for k in got:
            assert got[k].tobytes() == again[k].tobytes(), (c["name"], k)
    print("largest |lpb - float64| / bound over the table: %.3g" % worst)


def test_the_plan_names_both_row_kernels_and_both_load_widths_across_the_table(table):
    plans = [ops.ctc_blank_skip_plan(c["T"], c["B"], c["C"]) for c, _ in table]
    assert {p["kernel"] for p in plans} == {"wave", "block"} and {p["vec"] for p in plans} == {1, 4}
    assert {(p["kernel"], p["words_per_lane"]) for p in plans} == {("wave", 4), ("wave", 8), ("wave", 16), ("block", 8), ("block", 16)}
    assert max(p["chunks"] for p in plans) == 3


@pytest.mark.parametrize("name", ["T9_B3_C80_mixed", "T257_B3_C5_seam", "T7_B3_C1025_mixed"])
def test_a_row_does_not_depend_on_its_place_in_the_batch(table, name):
    c, ref = next((c, r) for c, r in table if c["name"] == name)
    T, B, C = c["logits"].shape
    rng = np.random.RandomState(5)
    order = [2, 0, 1, 0, 2]                                                  # another B, the rows moved and repeated
    logits = np.ascontiguousarray(c["logits"][:, order])
    lengths = np.asarray(c["lengths"])[order]
    logits[:, 3] = R.make_frames(rng.rand(T, 1) < 0.5, C, 77)[:, 0]          # ... next to a row that was not there before
    got = _run(logits, lengths, c["theta"])
    first = _run(c["logits"], c["lengths"], c["theta"])
    for pos, b in enumerate(order):
        if pos == 3:
            continue
        assert got["out_lengths"][pos] == first["out_lengths"][b] == ref["out_lengths"][b]
        assert np.array_equal(got["src_frame"][pos], first["src_frame"][b])
        assert got["out_logits"][:, pos].tobytes() == first["out_logits"][:, b].tobytes()
        assert got["blank_logp"][:, pos].tobytes() == first["blank_logp"][:, b].tobytes()


def test_every_refused_argument_returns_its_status_and_launches_nothing():
    load = lib.load()
    T, B, C = 6, 3, 8
    x = torch.randn(T, B, C, device="cuda")
    n = torch.full((B,), T, device="cuda", dtype=torch.int32)
    out = torch.full((2 * T, B, C), 7.0, device="cuda")
    new_len = torch.full((B,), -9, device="cuda", dtype=torch.int32)
    src = torch.full((B, T), 12345, device="cuda", dtype=torch.int32)
    ws = torch.zeros(1024, device="cuda", dtype=torch.uint8)
    p = lambda t: ctypes.c_void_p(t.data_ptr() if t is not None else 0)      # noqa: E731
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(T=T, B=B, C=C, thr=-0.1, logits=x, lengths=n, out_logits=out, out_lengths=new_len, src_frame=src, ws=ws, offset=0):
        return load.amdspeech_ctc_blank_skip(stream, p(logits), p(lengths), T, B, C, thr, ctypes.c_void_p(out_logits.data_ptr() + offset)
                                             if out_logits is not None else p(None), p(out_lengths), p(src_frame), p(None), p(ws))

    EINVAL, EUNSUPPORTED = -1, -3
    refused = [
        (dict(T=0), EINVAL, "at least 1"), (dict(B=0), EINVAL, "at least 1"), (dict(C=1), EINVAL, "below 2"),
        (dict(C=4097), EUNSUPPORTED, "4096"), (dict(T=1 << 15, B=1 << 10, C=64), EUNSUPPORTED, "2^31"),
        (dict(thr=0.1), EINVAL, "at most 0"), (dict(thr=float("nan")), EINVAL, "finite"), (dict(thr=float("-inf")), EINVAL, "finite"),
        (dict(logits=None), EINVAL, "null"), (dict(lengths=None), EINVAL, "null"), (dict(out_logits=None), EINVAL, "null"),
        (dict(out_lengths=None), EINVAL, "null"), (dict(src_frame=None), EINVAL, "null"), (dict(ws=None), EINVAL, "null"),
        (dict(out_logits=x), EINVAL, "overlaps"), (dict(logits=out, out_logits=out, offset=4 * B * C), EINVAL, "overlaps"),
        (dict(offset=4), EINVAL, "16-byte"),
    ]
    for kw, status, word in refused:
        assert call(**kw) == status, kw
        assert word in load.amdspeech_last_error().decode(), (kw, load.amdspeech_last_error())
    torch.cuda.synchronize()
    assert (out == 7.0).all() and (new_len == -9).all() and (src == 12345).all()      # nothing was launched
    assert call() == 0 and call(thr=0.0) == 0
    torch.cuda.synchronize()
    assert (new_len >= 1).all() and (out[T:] == 7.0).all()
    for bad in (0.0, 1.5, -1.0, float("nan")):
        with pytest.raises(ValueError, match="probability"):
            ops.ctc_blank_skip(x, n, bad)


# ---------------------------------------------------------------- the key in a small model
L_, H_, D_, C_, B_, T_, U_ = 2, 64, 20, 30, 3, 40, 10


def _peaky_model(kind="forward"):
    """A small model whose engine writes the seeded peaky pattern over its logits at the end of every forward pass."""
    from models.AcousticModel import AcousticModel
    model = AcousticModel(L_, H_, B_, T_, U_, D_, False, C_)
    if kind == "forward":
        model.create_forward_rnn()
    else:
        model.create_training_rnn(1.0, 1.0, 1.0, 1e-3, 0.5)
    pattern, _, _ = R.peaky_posteriors(T_, B_, C_, 0.75, seed=3)
    pattern = torch.from_numpy(pattern).cuda()
    forward = model.engine.forward

    def forward_then_pattern(*a, **kw):
        out = forward(*a, **kw)
        model.engine.logits.copy_(pattern)
        return out
    model.engine.forward = forward_then_pattern
    return model, pattern.cpu().numpy()


def _recorded(model, x, lens):
    import engine_calls
    rec = engine_calls.Recorder()
    with rec.recording():
        pred = model.process_input(None, x, lens)
    return pred, [e[0] for e in rec.entries]


def test_the_key_off_changes_nothing_and_on_decodes_the_same_strings_from_fewer_frames():
    model, pattern = _peaky_model()
    assert model.decode_blank_skip == 0.0
    rng = np.random.RandomState(2)
    x = rng.randn(T_, B_, D_).astype(np.float32)
    lens = np.array([40, 23, 0], np.int32)
    off, names_off = _recorded(model, x, lens)
    assert "ctc_blank_skip" not in names_off and names_off.count("ctc_beam_search") == 1 and model._skip_bufs is None
    ids, out_len, _ = ops.ctc_beam_search(pattern, lens, 100, True)          # what process_input returns today
    assert out_len[0] > 3 and out_len[2] == 0
    for b in range(B_):
        assert list(off[b][:out_len[b]]) == list(ids[b, :out_len[b]]) and np.all(off[b][out_len[b]:] == C_)
    # off hands the decoder the very objects it was given
    logits, dlen = model.engine.logits, torch.as_tensor(lens).cuda()
    got = model._decoder_input(logits, dlen)
    assert got[0] is logits and got[1] is dlen

    model.decode_blank_skip = 0.9
    on, names_on = _recorded(model, x, lens)
    assert names_on.count("ctc_blank_skip") == 1 and names_on.count("ctc_beam_search") == 1
    assert [n for n in names_on if n != "ctc_blank_skip"] == names_off
    assert on.shape == off.shape and np.array_equal(on, off)
    small, new_len = model._decoder_input(logits, dlen)
    ref = R.blank_skip_ref(pattern, lens, 0.9)
    assert not new_len.is_cuda and np.array_equal(new_len.numpy(), ref["out_lengths"]) and small.shape[0] == ref["out_lengths"].max() <= T_ // 2
    assert small.cpu().numpy().tobytes() == ref["out_logits"][:small.shape[0]].tobytes()

    model.decoder = "greedy"                                                 # the greedy decoder never skips
    _, names_greedy = _recorded(model, x, lens)
    assert "ctc_blank_skip" not in names_greedy and "ctc_greedy_decode" in names_greedy


def test_the_training_and_evaluation_decoders_skip_too_and_report_the_same_error_rate():
    """train_decoder : beam (the asynchronous decoder, lag 0 and lag 1) and an evaluation step (the synchronous one) with the key on
    report the error rate of the key off: the peaky pattern decodes to the same strings."""
    from models.AcousticModel import Session
    rng = np.random.RandomState(3)
    x = rng.randn(T_, B_, D_).astype(np.float32)
    lens = np.array([40, 31, 36], np.int32)
    dense = np.zeros((B_, U_), np.int32)
    for b in range(B_):
        dense[b, :4] = rng.randint(1, C_ - 1, size=4)
        dense[b, 4] = C_ - 1
    rates = {}
    for key in (0.0, 0.9):
        for lag in (0, 1):
            model, _ = _peaky_model("training")
            model.train_decoder, model.train_decoder_lag, model.decode_blank_skip = "beam", lag, key
            errs = []
            for _ in range(2):
                model.feed(x, lens, dense)
                errs.append(model.run_train_step(Session(), 1, 1.0)[1])
            rates[key, "train", lag] = errs
            if key:
                assert len(model._async_beam._len_bufs) >= 1
            else:
                assert not model._async_beam._len_bufs and model._skip_bufs is None
            if lag == 0:
                model.feed(x, lens, dense)
                model.start_batch(Session(), False)
                model.run_step(Session(), False)
                rates[key, "eval"] = model.end_batch(Session(), False)[1]
            model.close()
    assert rates[0.0, "train", 0][0] > 0
    assert rates[0.9, "train", 0] == rates[0.0, "train", 0] and rates[0.9, "train", 1] == rates[0.0, "train", 1]
    assert rates[0.9, "eval"] == rates[0.0, "eval"] == rates[0.0, "train", 0][0]
