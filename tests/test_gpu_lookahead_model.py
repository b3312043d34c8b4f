"""Engine(lookahead=...) against the float64 oracle with the row convolution between the top LSTM layer and the output layer
(tests/lookahead_ref.py: model_oracle), with the tolerances of tests/test_gpu_model.py::test_forward_backward_adam_parity; dropout
on with the library's own masks as tests/test_gpu_dropout_oracle.py feeds them; identity taps change nothing; clip + Adam moves
the taps; a checkpoint on the device reproduces the logits bit for bit."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lookahead_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu

from oracle import model as om  # noqa: E402  (checker only)


def rel_err(a, b):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-30))


def make_batch(T, B, D, C, U, seed):
    """Ragged lengths in T/2 .. T with one empty row, labels that fit (tests/test_gpu_model.py: make_batch)."""
    rng = np.random.RandomState(seed)
    x = rng.randn(T, B, D).astype(np.float32)
    lengths = rng.randint(min(max(2, T // 2), T), T + 1, size=B).astype(np.int32)
    if B > 2:
        lengths[1] = 0
    dense = np.zeros((B, U), np.int32)
    for b in range(B):
        n = rng.randint(1, max(2, min(U - 1, int(lengths[b]) // 3 + 1)))
        dense[b, :n] = rng.randint(1, C - 1, size=n)
        dense[b, n] = C - 1
    return x, lengths, dense


def engine_masks(ws, L):
    """(in_masks, out_masks) as float64 numpy [T,B,H] per layer, exported by the library for the descriptor of `ws`
    (tests/test_gpu_dropout_oracle.py: engine_masks)."""
    from rnn_speech_amd import ops
    ins = [ops.lstm_dropout_multipliers(ws, "in", l).cpu().numpy().astype(np.float64) for l in range(L)]
    outs = [ops.lstm_dropout_multipliers(ws, "out", l).cpu().numpy().astype(np.float64) for l in range(L)]
    return ins, outs


def _engine(L, H, D, C, B, T, U, context, seed=7, rng_seed=1):
    """An engine with random taps and non-zero biases, its parameters as float32 numpy and the device batch."""
    from rnn_speech_amd.engine import Engine
    eng = Engine(L, H, D, C, B, T, U, seed=seed, lookahead=context)
    rng = np.random.RandomState(rng_seed)
    p = eng.to_numpy()
    for k in p:
        if p[k].ndim == 1:
            p[k] = (rng.randn(*p[k].shape) * 0.1).astype(np.float32)
    p["lookahead_w"] = (rng.randn(context + 1, H) / np.sqrt(context + 1)).astype(np.float32)
    eng.load_numpy(p)
    return eng, p


def _device(x, lengths, dense):
    return torch.as_tensor(x).cuda(), torch.as_tensor(lengths).cuda(), torch.as_tensor(dense).cuda()


CONFIGS = [
    # L, H, D, C, B, T, U, context
    (1, 16, 8, 80, 2, 12, 6, 3),
    (2, 32, 20, 80, 5, 25, 10, 7),
    (3, 64, 40, 80, 33, 40, 16, 2),
    (3, 512, 40, 80, 32, 16, 8, 20),       # context > T
]


@pytest.mark.parametrize("L,H,D,C,B,T,U,context", CONFIGS)
def test_forward_backward_adam_parity_with_lookahead(L, H, D, C, B, T, U, context):
    eng, p = _engine(L, H, D, C, B, T, U, context)
    x, lengths, dense = make_batch(T, B, D, C, U, seed=L * 100 + H)
    dx, dlen, dlab = _device(x, lengths, dense)
    p64 = {k: v.astype(np.float64) for k, v in p.items()}
    logits_ref, loss_ref, g_ref = ref.model_oracle(om, p64, x, lengths, dense, L, C)

    eng.zero_grads()
    eng.mini_batch(dx, dlen, dlab)
    torch.cuda.synchronize()
    eng.check()
    path = eng.kernel_path()
    assert path["lookahead"] == context and path["fused_ctc_head"] is False, path
    logits = eng.logits.cpu().numpy()
    assert rel_err(logits, logits_ref) < 1e-4
    np.testing.assert_allclose(eng.loss.cpu().numpy(), loss_ref, rtol=1e-3, atol=1e-5)
    g = eng.to_numpy(eng.grads)
    assert sorted(g) == sorted(g_ref)
    for k in g_ref:
        assert rel_err(g[k], g_ref[k]) < 2e-3, (k, rel_err(g[k], g_ref[k]))
    from rnn_speech_amd import ops
    ids, out_len = ops.ctc_greedy_decode(eng.logits, dlen)
    ref_ids = om.greedy_decode(logits_ref, lengths)
    ids, out_len = ids.cpu().numpy(), out_len.cpu().numpy()
    for b in range(B):
        assert list(ids[b, :out_len[b]]) == ref_ids[b]
    # the taps matter: with identity taps the logits are another function
    plain, _, _ = om.forward({k: v for k, v in p64.items() if k != "lookahead_w"}, x.astype(np.float64), lengths, L)
    assert rel_err(plain, logits_ref) > 1e-2

    # one clip + Adam step moves the taps as the oracle's optimiser moves them (test_gpu_model's scaling of the tolerance)
    m = {k: np.zeros_like(v) for k, v in p64.items()}
    v = {k: np.zeros_like(vv) for k, vv in p64.items()}
    pn = {k: vv.copy() for k, vv in p64.items()}
    gn = om.clip_and_adam(pn, g_ref, m, v, 1, 3e-4, 1.0)
    norm = eng.apply(3e-4, 1.0)
    assert abs(float(norm.cpu()) - gn) <= 2e-3 * gn + 1e-12
    pd = eng.to_numpy()
    assert np.abs(pd["lookahead_w"] - p["lookahead_w"]).max() > 0.5 * 3e-4
    for k in pn:
        sure = np.abs(g_ref[k]) > 1e-3 * np.abs(g_ref[k]).max()
        if sure.any():
            assert np.abs((pd[k] - p[k]) - (pn[k] - p64[k]))[sure].max() < 0.05 * 3e-4, k
        else:                                   # (an all-zero gradient: nothing moves)
            assert np.abs(pd[k] - p[k]).max() < 1e-9, k


def test_dropout_on_training_step_with_lookahead_matches_oracle():
    L, H, D, C, B, T, U, context = 2, 64, 20, 80, 5, 25, 10, 4
    eng, p = _engine(L, H, D, C, B, T, U, context, rng_seed=2)
    x, lengths, dense = make_batch(T, B, D, C, U, seed=L * 100 + H)
    dx, dlen, dlab = _device(x, lengths, dense)
    with eng.on_stream():
        eng.zero_grads()
        eng.mini_batch(dx, dlen, dlab, 0.8, 0.5, seed=4242)
    torch.cuda.synchronize()
    eng.check()
    assert eng.kernel_path()["lookahead"] == context and not eng.kernel_path()["fused_ctc_head"]
    in_masks, out_masks = engine_masks(eng._ws, L)
    p64 = {k: v.astype(np.float64) for k, v in p.items()}
    logits_ref, loss_ref, g_ref = ref.model_oracle(om, p64, x, lengths, dense, L, C, in_masks=in_masks, out_masks=out_masks)
    assert rel_err(eng.logits.cpu().numpy(), logits_ref) < 1e-4
    np.testing.assert_allclose(eng.loss.cpu().numpy(), loss_ref, rtol=1e-3, atol=1e-5)
    g = eng.to_numpy(eng.grads)
    for k in g_ref:
        assert rel_err(g[k], g_ref[k]) < 2e-3, (k, rel_err(g[k], g_ref[k]))
    no_mask, _, _ = ref.model_oracle(om, p64, x, lengths, dense, L, C)
    assert rel_err(no_mask, logits_ref) > 1e-2


def test_identity_taps_leave_the_inference_logits_unchanged():
    from rnn_speech_amd.engine import Engine
    L, H, D, C, B, T, U = 2, 128, 20, 80, 6, 30, 8
    x, lengths, _ = make_batch(T, B, D, C, U, seed=3)
    dx, dlen = torch.as_tensor(x).cuda(), torch.as_tensor(lengths).cuda()
    plain = Engine(L, H, D, C, B, T, U, seed=21)
    la = Engine(L, H, D, C, B, T, U, seed=21, lookahead=5)
    assert torch.equal(la.params[:plain.layout.total], plain.params)
    for max_len in (None, int(lengths.max())):
        a = plain.forward(dx, dlen, max_len=max_len).clone()
        b = la.forward(dx, dlen, max_len=max_len).clone()
        assert la.kernel_path()["lookahead"] == 5 and plain.kernel_path()["lookahead"] == 0
        assert torch.equal(a, b), max_len


def test_run_length_clamp_gives_the_same_gradients():
    """A batch whose longest row is shorter than the padded length: the convolution runs the clamped length like everything else."""
    L, H, D, C, B, T, U, context = 1, 32, 8, 80, 3, 40, 6, 6
    eng, p = _engine(L, H, D, C, B, T, U, context)
    x, _, dense = make_batch(T, B, D, C, U, seed=4)
    lengths = np.asarray([23, 0, 17], np.int32)
    dx, dlen, dlab = _device(x, lengths, dense)
    out = []
    for max_len in (None, 23):
        eng.zero_grads()
        eng.mini_batch(dx, dlen, dlab, max_len=max_len)
        torch.cuda.synchronize()
        assert eng.kernel_path()["run_length"] == (T if max_len is None else 23)
        out.append((eng.logits.cpu().numpy().copy(), eng.to_numpy(eng.grads)))
    assert rel_err(out[1][0], out[0][0]) < 1e-6          # (another row count: the output GEMM may split differently)
    for k in out[0][1]:
        assert rel_err(out[1][1][k], out[0][1][k]) < 1e-5, k
    p64 = {k: v.astype(np.float64) for k, v in p.items()}
    _, _, g_ref = ref.model_oracle(om, p64, x, lengths, dense, L, C)
    assert rel_err(out[1][1]["lookahead_w"], g_ref["lookahead_w"]) < 2e-3


def test_checkpoint_on_the_device_reproduces_the_logits(tmp_path):
    from rnn_speech_amd import checkpoint
    from rnn_speech_amd.engine import Engine
    L, H, D, C, B, T, U, context = 2, 32, 20, 80, 4, 20, 8, 3
    eng, _ = _engine(L, H, D, C, B, T, U, context)
    x, lengths, dense = make_batch(T, B, D, C, U, seed=5)
    dx, dlen, dlab = _device(x, lengths, dense)
    eng.zero_grads()
    eng.mini_batch(dx, dlen, dlab)
    eng.apply(3e-4, 1.0)                                   # (non-zero Adam slots for the taps too)
    want = eng.forward(dx, dlen).clone()
    path = str(tmp_path / "la.npz")
    checkpoint.write(path, checkpoint.pack(eng, 3, 1e-3))
    z = np.load(path)
    assert np.any(z["adam/m/Lookahead_Layer/lookahead_w"] != 0)
    back = Engine(L, H, D, C, B, T, U, seed=99, lookahead=context)
    assert checkpoint.unpack(z, back)[2] is True
    assert torch.equal(back.params, eng.params) and torch.equal(back.adam_m, eng.adam_m) and torch.equal(back.adam_v, eng.adam_v)
    assert torch.equal(back.forward(dx, dlen), want)


def test_engine_refuses_lookahead_with_a_bidirectional_stack_or_out_of_range():
    from rnn_speech_amd.engine import Engine
    with pytest.raises(ValueError, match="bidirectional"):
        Engine(1, 16, 8, 80, 2, 12, 6, bidirectional=True, lookahead=3)
    with pytest.raises(ValueError, match=r"0 \(off\) .. 32"):
        Engine(1, 16, 8, 80, 2, 12, 6, lookahead=33)
