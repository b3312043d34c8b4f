"""GPU tests at BASELINE.json configs[2] full size (5x1024 LSTM, 120-dim fbank+delta+delta-delta, batch 64,
T = 998 frames = 10 s at 16 kHz): logits, CTC loss and EVERY gradient tensor against the float64 oracle on a
live pair of utterances, and the fbank front end at B = 64 x 10 s against the oracle."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import frontend as ofe  # noqa: E402  (checker only)
from oracle import model as om      # noqa: E402  (checker only)

L, H, D, C, B, T, U = 5, 1024, 120, 80, 64, 998, 161


def _rel(a, b):
    return float(np.abs(np.asarray(a, np.float64) - b).max() / (np.abs(b).max() + 1e-30))


def test_cfg3_full_length_logits_loss_and_gradients_match_oracle():
    from rnn_speech_amd.engine import Engine
    eng = Engine(L, H, D, C, B, T, U, seed=4321)
    rng = np.random.RandomState(11)
    p = eng.to_numpy()
    for k in p:
        if p[k].ndim == 1:
            p[k] = (rng.randn(*p[k].shape) * 0.1).astype(np.float32)
    eng.load_numpy(p)
    x = rng.randn(T, B, D).astype(np.float32)
    sel = [0, 41]                                          # rows of two different 16-row batch tiles
    lengths = np.zeros(B, np.int32)
    lengths[0], lengths[41] = T, 871
    dense = np.zeros((B, U), np.int32)
    for b in range(B):
        n = rng.randint(80, 161)
        dense[b, :n - 1] = rng.randint(1, C - 1, size=n - 1)
        dense[b, n - 1] = C - 1
    p64 = {k: v.astype(np.float64) for k, v in p.items()}
    logits_ref, _, cache = om.forward(p64, x[:, sel, :].astype(np.float64), lengths[sel], L, keep_cache=True)
    loss_ref, dl = om.ctc_loss_and_grad(logits_ref, om.sparsify_labels(dense[sel], C), lengths[sel])
    g_ref = om.backward(p64, cache, dl, lengths[sel], L)
    with eng.on_stream():
        eng.zero_grads()
        eng.mini_batch(torch.as_tensor(x).cuda(), torch.as_tensor(lengths).cuda(), torch.as_tensor(dense).cuda())
    torch.cuda.synchronize()
    eng.check()
    assert _rel(eng.logits.cpu().numpy()[:, sel, :], logits_ref) < 1e-4
    np.testing.assert_allclose(eng.loss.cpu().numpy()[sel], loss_ref, rtol=1e-3)
    assert not eng.loss.cpu().numpy()[[1, 40, 63]].any()
    g = eng.to_numpy(eng.grads)
    for k in g_ref:
        assert _rel(g[k], g_ref[k]) < 2e-3, (k, _rel(g[k], g_ref[k]))
    from rnn_speech_amd import ops
    ids, out_len = ops.ctc_greedy_decode(eng.logits, torch.as_tensor(lengths).cuda())
    ids, out_len = ids.cpu().numpy(), out_len.cpu().numpy()
    ref_ids = om.greedy_decode(logits_ref, lengths[sel])
    for j, b in enumerate(sel):
        assert list(ids[b, :out_len[b]]) == ref_ids[j]


def _synth(seed, n, sr):
    rng = np.random.RandomState(seed)
    t = np.arange(n) / float(sr)
    sig = 0.1 * rng.randn(n)
    for f0, a in ((220.0, 0.3), (1330.0, 0.2), (3100.0, 0.1)):
        sig += a * np.sin(2 * np.pi * f0 * (1 + 0.01 * (seed % 17)) * t)
    return sig.astype(np.float32)


def test_fbank_front_end_at_full_batch_matches_oracle():
    """B = 64 utterances of 10 s at 16 kHz -> [998, 64, 120]; every 9th row (and the ragged ones) against the
    oracle (static dims pinned by the reference's own numpy body, tests/golden/fbank_*.npz)."""
    from rnn_speech_amd.audioprocessor import AudioProcessor
    sr, n = 16000, 160000
    ap = AudioProcessor(T, "fbank")
    sigs = [_synth(b, n, sr) for b in range(B)]
    sigs[5] = sigs[5][:91234]                              # ragged rows
    sigs[63] = sigs[63][:40000]
    feat, lengths = ap.process_batch(sigs, sr)
    assert feat.shape == (T, B, D)
    assert lengths[0] == T and lengths[5] < T and lengths[63] < lengths[5]
    feat = feat.cpu().numpy()
    for b in list(range(0, B, 9)) + [5, 63]:
        ref = ofe.fbank(sigs[b].astype(np.float64), sr)
        assert lengths[b] == len(ref)
        nb = min(len(ref), T)
        # dB-scale values (|x| up to ~60) from an f32 DFT + log10; over 64 x 998 x 120 values the worst element of the
        # quiet frames reaches 2.5e-3 where the short-signal tests stay under 2e-3
        assert np.abs(feat[:nb, b] - ref[:nb]).max() < 5e-3, b
        assert not feat[nb:, b].any()


def test_cfg5_bidirectional_bf16x3_full_length_matches_oracle():
    """BASELINE configs[4]'s per-GPU share: 5x1024 BIDIRECTIONAL, 120-dim features, B = 64, T = 998, split-precision (bf16x3)
    products -- the two options combined, at full length, on a live pair of utterances against the float64 oracle: logits,
    CTC loss and every gradient tensor of both stacks."""
    from rnn_speech_amd.engine import Engine
    eng = Engine(L, H, D, C, B, T, U, seed=99, precision="bf16x3", bidirectional=True)
    rng = np.random.RandomState(12)
    p = eng.to_numpy()
    for k in p:
        if p[k].ndim == 1:
            p[k] = (rng.randn(*p[k].shape) * 0.1).astype(np.float32)
    eng.load_numpy(p)
    x = rng.randn(T, B, D).astype(np.float32)
    sel = [7, 50]
    lengths = np.zeros(B, np.int32)
    lengths[7], lengths[50] = 913, T
    dense = np.zeros((B, U), np.int32)
    for b in range(B):
        n = rng.randint(80, 161)
        dense[b, :n - 1] = rng.randint(1, C - 1, size=n - 1)
        dense[b, n - 1] = C - 1
    p64 = {k: v.astype(np.float64) for k, v in p.items()}
    logits_ref, cache = om.forward_bidirectional(p64, x[:, sel, :].astype(np.float64), lengths[sel], L)
    loss_ref, dl = om.ctc_loss_and_grad(logits_ref, om.sparsify_labels(dense[sel], C), lengths[sel])
    g_ref = om.backward_bidirectional(p64, cache, dl, lengths[sel], L)
    with eng.on_stream():
        eng.zero_grads()
        eng.mini_batch(torch.as_tensor(x).cuda(), torch.as_tensor(lengths).cuda(), torch.as_tensor(dense).cuda())
    torch.cuda.synchronize()
    eng.check()
    assert not eng.kernel_path()["paired"]       # (split precision keeps W_hh on XCD pairs: two calls, lstm_fwd_big<1> / lstm_bwd_big<1>)
    assert (eng.kernel_path()["lstm_fwd"], eng.kernel_path()["lstm_bwd"]) == ("big", "big")
    assert _rel(eng.logits.cpu().numpy()[:, sel, :], logits_ref) < 1e-3          # north_star's bound; f32 path: 1e-4
    np.testing.assert_allclose(eng.loss.cpu().numpy()[sel], loss_ref, rtol=1e-3)
    g = eng.to_numpy(eng.grads)
    for k in g_ref:
        assert _rel(g[k], g_ref[k]) < 5e-3, (k, _rel(g[k], g_ref[k]))


@pytest.mark.parametrize("bidirectional", [False, True], ids=["unidirectional", "bidirectional"])
def test_cfg5_plain_bf16_error_over_998_frames_is_what_the_study_says(bidirectional):
    """precision = "bf16" (round 4: ONE bf16 per operand value, one MFMA per product, f32 accumulation / gates / state / master
    weights -- BASELINE configs[4]'s "bf16 MFMA") at 5x1024, B = 64, T = 998 on a live pair against the float64 oracle.  The bounds
    are what the mode MEETS (tools/bf16_error_study.py: logits 1.3-1.9e-3 of max, loss 7e-5, gradients 3.7-4.8e-3), with margin:
    the logits are OUTSIDE north_star's 1e-3 -- which is why the mode is opt-in and never the headline -- the CTC loss is inside."""
    from rnn_speech_amd.engine import Engine
    eng = Engine(L, H, D, C, B, T, U, seed=99, precision="bf16", bidirectional=bidirectional)
    rng = np.random.RandomState(12)
    p = eng.to_numpy()
    for k in p:
        if p[k].ndim == 1:
            p[k] = (rng.randn(*p[k].shape) * 0.1).astype(np.float32)
    eng.load_numpy(p)
    x = rng.randn(T, B, D).astype(np.float32)
    # a live row in EVERY 16-row batch tile: the one-XCD pair kernels place tile i of stack 0 on XCD i and of stack 1 on XCD 4 + i, so
    # all eight XCDs' groups reach the oracle directly (rows 7 and 50 alone left tiles 1-2 to the T <= 64 comparisons of test_gpu_lstm_pair.py)
    sel = [7, 20, 41, 50]
    lengths = np.zeros(B, np.int32)
    lengths[7], lengths[20], lengths[41], lengths[50] = 913, T, 677, T
    dense = np.zeros((B, U), np.int32)
    for b in range(B):
        n = rng.randint(80, 161)
        dense[b, :n - 1] = rng.randint(1, C - 1, size=n - 1)
        dense[b, n - 1] = C - 1
    p64 = {k: v.astype(np.float64) for k, v in p.items()}
    if bidirectional:
        logits_ref, cache = om.forward_bidirectional(p64, x[:, sel, :].astype(np.float64), lengths[sel], L)
    else:
        logits_ref, _, cache = om.forward(p64, x[:, sel, :].astype(np.float64), lengths[sel], L, keep_cache=True)
    loss_ref, dl = om.ctc_loss_and_grad(logits_ref, om.sparsify_labels(dense[sel], C), lengths[sel])
    g_ref = (om.backward_bidirectional if bidirectional else om.backward)(p64, cache, dl, lengths[sel], L)
    with eng.on_stream():
        eng.zero_grads()
        eng.mini_batch(torch.as_tensor(x).cuda(), torch.as_tensor(lengths).cuda(), torch.as_tensor(dense).cuda())
    torch.cuda.synchronize()
    eng.check()
    # the kernels this test is about: both stacks' layers side by side on one-XCD groups (lstm_fwd_big1 / lstm_bwd_big1<4> through
    # amdspeech_lstm_fwd_pair / _bwd_pair) when bidirectional, never for one stack
    assert eng.kernel_path()["paired"] == bidirectional
    # ... by the library's own plan (ops.lstm_plan).  One stack alone runs forward on the XCD pairs; its backward recurrence takes
    # the one-XCD kernel whenever the bf16 operand copies are used (the switch test below runs this case without them)
    copies = os.environ.get("AMDSPEECH_BF16_PACKED", "1") != "0"
    assert eng.kernel_path()["lstm_fwd"] == ("big1" if bidirectional else "big")
    assert eng.kernel_path()["lstm_bwd"] == ("big1" if copies else "big")
    e_logits = _rel(eng.logits.cpu().numpy()[:, sel, :], logits_ref)
    assert 2e-4 < e_logits < 5e-3, e_logits            # (really bf16: the split-precision mode sits at 3e-6)
    np.testing.assert_allclose(eng.loss.cpu().numpy()[sel], loss_ref, rtol=1e-3)
    g = eng.to_numpy(eng.grads)
    for k in g_ref:
        assert _rel(g[k], g_ref[k]) < 1.5e-2, (k, _rel(g[k], g_ref[k]))


def test_plain_bf16_without_operand_copies_keeps_the_bounds():
    """AMDSPEECH_BF16_PACKED=0: the batched products of precision = "bf16" on gemm_bf16 (f32 operands converted on the
    way into LDS, round 4) instead of bf16 operand copies + the global_load_lds kernel (round 5): the same full-length bounds, in a
    child process (the library reads the switch once)."""
    import os
    import subprocess
    import sys
    out = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-m", "gpu", "-q", "-x", "-k",
                          "test_cfg5_plain_bf16_error_over_998_frames_is_what_the_study_says and unidirectional"],
                         env=dict(os.environ, AMDSPEECH_BF16_PACKED="0"), capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-2000:]

