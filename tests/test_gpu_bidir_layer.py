"""Layer-wise bidirectional stacks (bidirectional_mode = layer, amdspeech_lstm_bidir_*) on the GPU against a float64 reference:
logits, CTC loss and every gradient tensor, through the C ABI and the engine."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import model as om  # noqa: E402  (checker only)

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bidir_layer_ref as ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def rel_err(a, b):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-30))


def make_batch(T, B, D, C, U, seed, edge_lengths=False):
    rng = np.random.RandomState(seed)
    x = rng.randn(T, B, D).astype(np.float32)
    lengths = rng.randint(max(1, T // 2), T + 1, size=B).astype(np.int32)
    if edge_lengths:
        lengths[:3] = [0, 1, T]
    dense = np.zeros((B, U), np.int32)
    for b in range(B):
        n = rng.randint(1, max(2, min(U - 1, int(lengths[b]) // 3 + 1)))
        dense[b, :n] = rng.randint(1, C - 1, size=n)
        dense[b, n] = C - 1
    return x, lengths, dense


def make_engine(L, H, D, C, B, T, U, seed=9, **kw):
    from rnn_speech_amd.engine import Engine
    eng = Engine(L, H, D, C, B, T, U, seed=seed, bidirectional=True, bidirectional_mode="layer", **kw)
    rng = np.random.RandomState(seed + 1)
    p = eng.to_numpy()
    for k in p:
        if p[k].ndim == 1:
            p[k] = (rng.randn(*p[k].shape) * 0.1).astype(np.float32)
    eng.load_numpy(p)
    return eng, p


def run_case(L, H, B, T, D=40, C=80, U=8, edge=False, keep=(1.0, 1.0), expect_path="persistent"):
    eng, p = make_engine(L, H, D, C, B, T, U)
    x, lengths, dense = make_batch(T, B, D, C, U, seed=H + B + L, edge_lengths=edge)
    dx, dlen, dlab = torch.as_tensor(x).cuda(), torch.as_tensor(lengths).cuda(), torch.as_tensor(dense).cuda()
    eng.zero_grads()
    eng.mini_batch(dx, dlen, dlab, keep_in=keep[0], keep_out=keep[1], seed=77)
    torch.cuda.synchronize()
    eng.check()
    assert eng.kernel_path()["layer_recurrence"] == expect_path
    masks = None
    if keep != (1.0, 1.0):
        from rnn_speech_amd import ops
        masks = {(d, w, l): ops.lstm_bidir_dropout_multipliers(eng._ws, d, w, l).cpu().numpy()
                 for d in ("fw", "bw") for w in ("in", "out") for l in range(L)}
    sparse = om.sparsify_labels(dense, C)
    logits_ref, loss_ref, g_ref = ref.forward_backward(p, x, lengths, L, H, lambda lg: om.ctc_loss_and_grad(lg, sparse, lengths),
                                                       masks=masks, device="cuda")
    assert rel_err(eng.logits.cpu().numpy(), logits_ref) < 1e-4
    np.testing.assert_allclose(eng.loss.cpu().numpy(), loss_ref, rtol=1e-3, atol=1e-5)
    g = eng.to_numpy(eng.grads)
    for k in g_ref:
        assert rel_err(g[k], g_ref[k]) < 2e-3, (k, rel_err(g[k], g_ref[k]))
    return eng


@pytest.mark.parametrize("L,H,B,T,edge", [(2, 64, 3, 17, False), (3, 128, 20, 50, True), (2, 256, 32, 200, False)],
                         ids=["2x64", "3x128-edge-lengths", "2x256"])
def test_layerwise_parity(L, H, B, T, edge):
    run_case(L, H, B, T, edge=edge)


@pytest.mark.parametrize("L,H,B,T,D", [(3, 512, 32, 1001, 40), (5, 1024, 64, 998, 120)], ids=["3x512", "5x1024"])
def test_layerwise_parity_full_size(L, H, B, T, D):
    run_case(L, H, B, T, D=D, U=40)


def test_layerwise_dropout_with_exported_masks():
    run_case(2, 128, 12, 40, keep=(0.8, 0.5))


def test_one_layer_matches_top_joined_mode():
    from rnn_speech_amd.engine import Engine
    L, H, D, C, B, T, U = 1, 128, 40, 80, 9, 33, 8
    eng, p = make_engine(L, H, D, C, B, T, U)
    top = Engine(L, H, D, C, B, T, U, seed=9, bidirectional=True)
    top.load_numpy(p)
    x, lengths, dense = make_batch(T, B, D, C, U, seed=5)
    dx, dlen, dlab = torch.as_tensor(x).cuda(), torch.as_tensor(lengths).cuda(), torch.as_tensor(dense).cuda()
    for e in (eng, top):
        e.zero_grads()
        e.mini_batch(dx, dlen, dlab)
    torch.cuda.synchronize()
    assert rel_err(eng.logits.cpu().numpy(), top.logits.cpu().numpy()) < 1e-6
    ga, gb = eng.to_numpy(eng.grads), top.to_numpy(top.grads)
    for k in gb:
        assert rel_err(ga[k], gb[k]) < 1e-5, k


def test_per_frame_switch_gives_the_same_results():
    """AMDSPEECH_BIDIR_PERSISTENT=0 (a fresh process: the switch is read once) runs the per-frame launches."""
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r); import test_gpu_bidir_layer as t; "
            "t.run_case(2, 128, 12, 30, expect_path='per_frame'); print('ok')") % (ROOT, os.path.join(ROOT, "tests"))
    env = dict(os.environ, AMDSPEECH_BIDIR_PERSISTENT="0")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


@pytest.mark.parametrize("where", ["fwd", "bwd"])
def test_timeout_is_reported_and_repeat_succeeds(where):
    from rnn_speech_amd import ops, lib
    L, H, D, C, B, T, U = 2, 128, 40, 80, 8, 40, 8
    eng, p = make_engine(L, H, D, C, B, T, U)
    x, lengths, dense = make_batch(T, B, D, C, U, seed=3)
    dx, dlen = torch.as_tensor(x).cuda(), torch.as_tensor(lengths).cuda()
    ws = eng.lstm_ws
    ks, bs = eng._cells(eng.params)
    dks, dbs = eng._cells(eng.grads)
    ws.z0.normal_()
    ops.lstm_bidir_fwd(ws, ks, bs, dlen, inject_timeout=(where == "fwd"))
    if where == "bwd":
        torch.cuda.synchronize()
        ops.lstm_bidir_status(ws)
        ws.dytop_fw.normal_()
        ws.dytop_bw.normal_()
        ops.lstm_bidir_bwd(ws, ks, dks, dbs, dlen, inject_timeout=True)
    torch.cuda.synchronize()
    with pytest.raises(lib.DataflowTimeout):
        ops.lstm_bidir_status(ws)
    run_case(L, H, B, T)         # a fresh engine after the time-out: correct results
    ops.lstm_bidir_fwd(ws, ks, bs, dlen)
    ops.lstm_bidir_bwd(ws, ks, dks, dbs, dlen)
    torch.cuda.synchronize()
    ops.lstm_bidir_status(ws)


def test_reduced_precision_is_refused():
    from rnn_speech_amd.engine import Engine
    from rnn_speech_amd import ops, lib
    with pytest.raises(ValueError, match="f32"):
        Engine(2, 64, 20, 80, 3, 10, 4, bidirectional=True, bidirectional_mode="layer", precision="bf16")
    d = lib.LstmDesc(10, 3, 64, 2, 1.0, 1.0, 0, 2)
    import ctypes
    assert lib.load().amdspeech_lstm_bidir_workspace_bytes(ctypes.byref(d)) == 0
    assert lib.load().amdspeech_lstm_bidir_path(ctypes.byref(d)) == -3       # AMDSPEECH_EUNSUPPORTED


def test_engine_training_loss_falls_and_state_round_trips():
    L, H, D, C, B, T, U = 2, 64, 20, 30, 8, 30, 6
    eng, p = make_engine(L, H, D, C, B, T, U)
    x, lengths, dense = make_batch(T, B, D, C, U, seed=12)
    dx, dlen, dlab = torch.as_tensor(x).cuda(), torch.as_tensor(lengths).cuda(), torch.as_tensor(dense).cuda()
    losses = []
    for _ in range(20):
        eng.zero_grads()
        losses.append(float(eng.mini_batch(dx, dlen, dlab).sum()))
        eng.apply(3e-3, 5.0)
    torch.cuda.synchronize()
    eng.check()
    assert losses[-1] < 0.7 * losses[0], losses
    snap = eng.to_numpy()
    eng2, _ = make_engine(L, H, D, C, B, T, U, seed=1)
    eng2.load_numpy(snap)
    a = eng.forward(dx, dlen).clone()
    b = eng2.forward(dx, dlen).clone()
    torch.cuda.synchronize()
    assert torch.equal(a, b)
