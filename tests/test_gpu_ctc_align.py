"""The CTC aligner (amdspeech_ctc_align: csrc/ctc_align.h) on the GPU against tests/ctc_align_ref.py, over every case of the CTC
matrix (tests/ctc_ref.py: CASES) -- per row validity, optimality within a bound that comes from the reference's own arithmetic,
equality with the reference path frame by frame, and the confidences -- then the loss call beside it on another stream, the model
level (Engine.align on the uni-directional and the layer-wise bidirectional stack) and the drop-in class with the command line.

Optimality is tie-proof: what is held against the bound is the float64 score of the path the device RETURNED.  Equality allows a
stretch of frames to differ only where it begins (seen from the end) at a decision whose float64 margin is below the row's bound;
the count of such frames is printed per case and each such stretch still has to pass optimality."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ctc_align_ref as A  # noqa: E402
import ctc_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_align(logits, dense, lengths):
    from rnn_speech_amd import ops
    out = ops.ctc_align(torch.as_tensor(logits).cuda(), torch.as_tensor(dense).cuda(), torch.as_tensor(lengths).cuda())
    torch.cuda.synchronize()
    return {k: getattr(out, k).cpu().numpy() for k in ("frame_label", "frame_state", "spans", "score", "confidence")}


def check_rows(name, logits, dense, lengths, got):
    """Criteria 1-4 on every row of a batch; -> number of frames the equality exception covered."""
    T, B, C = logits.shape
    U = dense.shape[1]
    ref = A.align(logits, dense, lengths)
    emu = A.align(logits, dense, lengths, emulate=True)
    excepted = 0
    for b, (r, e) in enumerate(zip(ref, emu)):
        fs, fl, sp, sc, cf = got["frame_state"][b], got["frame_label"][b], got["spans"][b], got["score"][b], got["confidence"][b]
        where = "%s row %d" % (name, b)
        if r is None or r["path"] is None:
            # rows the loss ignores: score exactly 0; rows without an alignment: -inf; -1 in every frame and span
            assert (sc == 0.0 and not np.signbit(sc)) if r is None else np.isneginf(sc), (where, sc)
            assert (fs == -1).all() and (fl == -1).all() and (sp == -1).all() and (cf == 0).all(), where
            continue
        Tb, ext, skip, tgt, lp = r["Tb"], r["ext"], r["skip"], r["tgt"], r["lp"]
        n = len(tgt)
        # ---- 1. validity
        assert (fs[Tb:] == -1).all() and (fl[Tb:] == -1).all(), where
        path = fs[:Tb].astype(np.int64)
        assert path.min() >= 0 and path.max() < len(ext), where
        assert not A.validity(path, ext, skip, tgt, C), (where, A.validity(path, ext, skip, tgt, C))
        assert (fl[:Tb] == ext[path]).all(), where
        want_spans, want_conf = A.spans_conf(path, lp, ext, n)
        assert (sp[:n] == want_spans).all() and (sp[n:] == -1).all(), where
        assert (cf[n:] == 0).all(), where
        # ---- 2. optimality of the RETURNED path, and the returned score against its own path
        bound = A.bound(r, e)
        own = A.path_score(lp, ext, path)
        print("%s: Tb %d S %d  best %.6f  own path %.6f (short by %.2e)  returned %.6f (off its path by %.2e)  bound %.2e  emulated error %.2e"
              % (where, Tb, len(ext), r["score"], own, r["score"] - own, sc, abs(float(sc) - own), bound, abs(e["score"] - r["score"])))
        assert own <= r["score"] + 1e-9 * abs(r["score"]), where      # (nothing beats the best)
        assert r["score"] - own <= bound, (where, r["score"] - own, bound)
        assert abs(float(sc) - own) <= bound, (where, float(sc), own, bound)
        # ---- 3. equality, frame by frame
        for ta, tb in A.differing_stretches(path, r["path"]):
            margin = A.stretch_margin(r, tb)
            print("%s: frames %d..%d differ from the reference path; the decision they begin at has margin %.3e (bound %.3e)" % (where, ta, tb, margin, bound))
            assert margin < bound, (where, ta, tb, margin, bound)
            excepted += tb - ta + 1
        # ---- 4. confidence on the device's own path
        rel = np.abs(cf[:n] - want_conf) / want_conf
        if n:
            print("%s: confidence, largest relative error %.2e" % (where, rel.max()))
        assert (rel <= 1e-5).all(), (where, rel.max())
    return excepted


@pytest.mark.parametrize("name", [c["name"] for c in R.CASES])
def test_align_matrix(name):
    from rnn_speech_amd import ops
    c = R.by_name(name)
    logits, dense, lengths, info = R.build(c)
    kernel, rmax, threads = A.expected_plan(c["U"])
    assert ops.ctc_align_plan(c["T"], c["B"], c["C"], c["U"]) == {"kernel": kernel, "threads": threads, "rmax": rmax, "smax": 2 * c["U"] + 1}
    got = run_align(logits, dense, lengths)
    for b, i in enumerate(info):                     # the matrix's own bookkeeping agrees with what came back
        if not i["valid"]:
            assert got["score"][b] == 0.0
        elif i["inf"]:
            assert np.isneginf(got["score"][b])
        else:
            assert np.isfinite(got["score"][b]) and got["score"][b] < 0
    excepted = check_rows(name, logits, dense, lengths, got)
    print("%s: %d frames under the equality exception" % (name, excepted))


def test_matrix_holds_the_shapes_the_issue_names():
    """T = 1, 2, 7, 8, 9; B = 1; C = 3 and C = 4096: all cases of the matrix above."""
    names = {c["name"] for c in R.CASES}
    assert {"T%d-U%d" % (T, U) for T in (1, 2, 7, 8, 9) for U in (12, 100, 200, 300)} <= names
    assert {"single-U150", "single-U250", "single-U500", "C3-wave", "C3-wide", "C4096-wave", "C4096-wide"} <= names
    assert R.by_name("single-U150")["B"] == 1


def test_all_equal_logits_follow_the_tie_rule():
    """Ties everywhere: the device's path is the reference's, frame for frame, on a one-wave and on a four-wave shape."""
    for T, C, U, tgts in ((9, 6, 5, [[1, 2], [3, 3, 1], [4], []]), (40, 6, 70, [[1, 2, 3, 4] * 8, [2, 2, 2], [1] * 20])):
        dense = np.zeros((len(tgts), U), np.int32)
        for b, t in enumerate(tgts):
            dense[b, :len(t)] = t
        lengths = np.full(len(tgts), T, np.int32)
        logits = np.zeros((T, len(tgts), C), np.float32)
        got = run_align(logits, dense, lengths)
        ref = A.align(logits, dense, lengths)
        for b, r in enumerate(ref):
            if r["path"] is None:
                assert np.isneginf(got["score"][b])
                continue
            assert (got["frame_state"][b][:T] == r["path"]).all(), (T, b, got["frame_state"][b][:T], r["path"])
            assert abs(got["score"][b] - r["score"]) <= 1e-5 * abs(r["score"])


def test_aligner_on_a_side_stream_leaves_the_loss_bit_identical():
    """The aligner has its own workspace: an alignment on a non-default stream followed by the loss on the same logits gives the
    loss and gradient of a run without the aligner, bit for bit, and the alignment is the one a lone call returns."""
    from rnn_speech_amd import ops
    c = R.by_name("shift-161")
    logits, dense, lengths, _ = R.build(c)
    lg, dn, ln = torch.as_tensor(logits).cuda(), torch.as_tensor(dense).cuda(), torch.as_tensor(lengths).cuda()
    ws = ops.CtcWorkspace(c["T"], c["B"], c["C"], c["U"])
    loss0, d0 = ops.ctc_loss_fwd_bwd(lg, dn, ln, ws=ws)
    torch.cuda.synchronize()
    loss0, d0 = loss0.clone(), d0.clone()
    alone = ops.ctc_align(lg, dn, ln)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        al = ops.ctc_align(lg, dn, ln)
    side.synchronize()
    loss1, d1 = ops.ctc_loss_fwd_bwd(lg, dn, ln, ws=ws)
    torch.cuda.synchronize()
    assert torch.equal(loss0, loss1) and torch.equal(d0, d1)
    for k in ("frame_label", "frame_state", "spans", "score", "confidence"):
        assert torch.equal(getattr(al, k), getattr(alone, k)), k


# ------------------------------------------------------------------------------------------------ model level
def _trained_engine(bidirectional_layer):
    """A 2 x 64 engine trained for 20 steps on one batch, as tests/test_gpu_bidir_layer.py trains its own."""
    from rnn_speech_amd.engine import Engine
    L, H, D, C, B, T, U = 2, 64, 20, 30, 8, 30, 6
    kw = dict(bidirectional=True, bidirectional_mode="layer") if bidirectional_layer else {}
    eng = Engine(L, H, D, C, B, T, U, seed=9, **kw)
    rng = np.random.RandomState(12)
    x = rng.randn(T, B, D).astype(np.float32)
    lengths = rng.randint(T // 2, T + 1, size=B).astype(np.int32)
    dense = np.zeros((B, U), np.int32)
    for b in range(B):
        n = rng.randint(1, U - 1)
        dense[b, :n] = rng.randint(1, C - 1, size=n)
        dense[b, n] = C - 1
    dx, dlen, dlab = torch.as_tensor(x).cuda(), torch.as_tensor(lengths).cuda(), torch.as_tensor(dense).cuda()
    for _ in range(20):
        eng.zero_grads()
        eng.mini_batch(dx, dlen, dlab)
        eng.apply(3e-3, 5.0)
    torch.cuda.synchronize()
    eng.check()
    return eng, (dx, dlen, dlab), (x, lengths, dense)


@pytest.mark.parametrize("layerwise", [False, True], ids=["unidirectional", "bidirectional-layer"])
def test_engine_align_is_valid_and_never_beats_the_loss(layerwise):
    eng, (dx, dlen, dlab), (x, lengths, dense) = _trained_engine(layerwise)
    al = eng.align(dx, dlen, dlab)
    torch.cuda.synchronize()
    eng.check()
    logits = eng.logits.cpu().numpy().copy()
    got = {k: getattr(al, k).cpu().numpy() for k in ("frame_label", "frame_state", "spans", "score", "confidence")}
    check_rows("engine", logits, dense, lengths, got)
    eng.zero_grads()
    loss = eng.mini_batch(dx, dlen, dlab).cpu().numpy()      # (no dropout by default: the same logits)
    torch.cuda.synchronize()
    assert np.isfinite(got["score"]).all() and (got["score"] < 0).all()
    # the best path cannot beat the sum over all paths; both sides are float32 roundings of their sums, hence one ulp each
    slack = 2 * np.spacing(np.abs(loss).astype(np.float32))
    print("score", got["score"], "-loss", -loss)
    assert (got["score"] <= -loss + slack).all(), (got["score"], -loss)


# ------------------------------------------------------------------------------------------------ the drop-in class and the command line
def test_acoustic_model_align_and_stt_align_mode(tmp_path, monkeypatch, capsys):
    import test_gpu_stt as S
    d = str(tmp_path)
    texts = ["hello there", "good bye", "it'll do", "yes", "no way", "well-being"]
    with open(os.path.join(d, "train.tsv"), "w") as tr, open(os.path.join(d, "test.tsv"), "w") as te:
        for i, txt in enumerate(texts):
            S.write_wav(os.path.join(d, "u%d.wav" % i), i)
            (tr if i < 5 else te).write("%s\t%s\n" % (os.path.join(d, "u%d.wav" % i), txt))
    cfg = os.path.join(d, "config.ini")
    with open(cfg, "w") as fh:
        fh.write(S.CONFIG % {"dir": d})
    import stt
    monkeypatch.setattr(sys, "argv", ["stt.py", "--train_acoustic", "--config", cfg, "--max_epoch", "1"])
    stt.main()                                    # writes the checkpoint --align restores
    capsys.readouterr()
    from rnn_speech_amd.acoustic_model import AcousticModel
    seen = []
    plain = AcousticModel.align

    def spy(self, *a, **kw):
        seen.append(plain(self, *a, **kw))
        return seen[-1]
    monkeypatch.setattr(AcousticModel, "align", spy)
    seconds, frame_s = 0.5, 220 / 22050.0         # S.write_wav's duration; the front end's hop at 22,050 Hz
    for argv, text in ((["--transcript", "Hello there"], "hello there"), (["--transcript_file", os.path.join(d, "t.txt")], "it'll do")):
        with open(os.path.join(d, "t.txt"), "w") as fh:
            fh.write("It'll do.\n")
        monkeypatch.setattr(sys, "argv", ["stt.py", "--align", os.path.join(d, "u0.wav"), "--config", cfg] + argv)
        stt.main()
        lines = [ln.split() for ln in capsys.readouterr().out.strip().splitlines()]
        assert [ln[3] for ln in lines] == text.split(), lines
        times = [float(v) for ln in lines for v in ln[:2]]
        assert times == sorted(times) and times[0] >= 0 and times[-1] <= seconds, times
        assert all(0 < float(ln[2]) <= 1 for ln in lines)
        # AcousticModel.align itself: one utterance, (token, first_frame, last_frame, confidence) per token of the transcript
        tokens = seen[-1][0]
        ids = stt.dataprocessor.DataProcessor.get_str_labels(stt.SpeechRecognizer("english").get_char_map(), text, add_eos=False)
        assert [t[0] for t in tokens] == ids
        frames = [f for t in tokens for f in t[1:3]]
        assert frames == sorted(frames) and all(isinstance(t[3], float) and 0 < t[3] <= 1 for t in tokens)
        assert abs(times[0] - tokens[0][1] * frame_s) < 1e-3 and abs(times[-1] - tokens[-1][2] * frame_s) < 1e-3
