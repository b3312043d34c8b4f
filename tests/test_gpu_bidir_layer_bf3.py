"""Layer-wise bidirectional stacks in split precision (bidirectional_mode = layer, precision = bf16x3): the bf16-MFMA recurrence
kernels (csrc/lstm_layer_bf3.h) and the bf16x3 batched products, against the float64 reference -- logits, CTC loss and every
gradient tensor -- plus dropout, the per-frame launches, time-outs, training and the config.ini drop-in path."""
import json
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
import test_gpu_bidir_layer as base  # noqa: E402  (make_batch, make_engine, rel_err)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_case_bf3(L, H, B, T, D=40, C=80, U=8, edge=False, keep=(1.0, 1.0), expect_path="persistent", grad_bound=2e-3):
    eng, p = base.make_engine(L, H, D, C, B, T, U, precision="bf16x3")
    x, lengths, dense = base.make_batch(T, B, D, C, U, seed=H + B + L, edge_lengths=edge)
    dx, dlen, dlab = torch.as_tensor(x).cuda(), torch.as_tensor(lengths).cuda(), torch.as_tensor(dense).cuda()
    eng.zero_grads()
    eng.mini_batch(dx, dlen, dlab, keep_in=keep[0], keep_out=keep[1], seed=77)
    torch.cuda.synchronize()
    eng.check()
    path = eng.kernel_path()
    assert path["layer_product"] == "bf16x3" and path["layer_recurrence"] == expect_path, path
    masks = None
    if keep != (1.0, 1.0):
        from rnn_speech_amd import ops
        masks = {(d, w, l): ops.lstm_bidir_dropout_multipliers(eng._ws, d, w, l).cpu().numpy()
                 for d in ("fw", "bw") for w in ("in", "out") for l in range(L)}
    sparse = om.sparsify_labels(dense, C)
    logits_ref, loss_ref, g_ref = ref.forward_backward(p, x, lengths, L, H, lambda lg: om.ctc_loss_and_grad(lg, sparse, lengths),
                                                       masks=masks, device="cuda")
    loss = eng.loss.cpu().numpy()
    g = eng.to_numpy(eng.grads)
    errs = {"logits": base.rel_err(eng.logits.cpu().numpy(), logits_ref),
            "loss": float(np.max(np.abs(loss - loss_ref) / np.maximum(np.abs(loss_ref), 1e-30))),
            "grads": max(base.rel_err(g[k], g_ref[k]) for k in g_ref)}
    print("bf16x3 layer-wise errors", json.dumps(dict(errs, shape="%dx%d B%d T%d" % (L, H, B, T), keep=list(keep))))
    assert errs["logits"] < 1e-4, errs
    np.testing.assert_allclose(loss, loss_ref, rtol=1e-3, atol=1e-5)
    for k in g_ref:
        assert base.rel_err(g[k], g_ref[k]) < grad_bound, (k, base.rel_err(g[k], g_ref[k]))
    return eng


@pytest.mark.parametrize("L,H,B,T,edge", [(2, 64, 3, 17, False), (3, 128, 20, 50, True), (2, 256, 32, 200, False)],
                         ids=["2x64", "3x128-edge-lengths", "2x256"])
def test_bf3_layerwise_parity(L, H, B, T, edge):
    run_case_bf3(L, H, B, T, edge=edge)


@pytest.mark.parametrize("L,H,B,T,D", [(3, 512, 32, 1001, 40), (5, 1024, 64, 998, 120)], ids=["3x512", "5x1024"])
def test_bf3_layerwise_parity_full_size(L, H, B, T, D):
    run_case_bf3(L, H, B, T, D=D, U=40, grad_bound=5e-3)


def test_bf3_layerwise_dropout_with_exported_masks():
    run_case_bf3(2, 128, 12, 40, keep=(0.8, 0.5))


def test_bf3_per_frame_switch_meets_the_same_bounds():
    """AMDSPEECH_BIDIR_PERSISTENT=0 (a fresh process: the switch is read once): the bf16x3 kernels one frame per launch."""
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r); import test_gpu_bidir_layer_bf3 as t; "
            "t.run_case_bf3(2, 128, 12, 30, expect_path='per_frame'); t.run_case_bf3(2, 64, 3, 17, expect_path='per_frame'); "
            "print('ok')") % (ROOT, os.path.join(ROOT, "tests"))
    env = dict(os.environ, AMDSPEECH_BIDIR_PERSISTENT="0")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


@pytest.mark.parametrize("where", ["fwd", "bwd"])
def test_bf3_timeout_is_reported_and_next_step_is_correct(where):
    from rnn_speech_amd import ops, lib
    L, H, D, C, B, T, U = 2, 128, 40, 80, 8, 40, 8
    eng, p = base.make_engine(L, H, D, C, B, T, U, precision="bf16x3")
    x, lengths, dense = base.make_batch(T, B, D, C, U, seed=3)
    dlen = torch.as_tensor(lengths).cuda()
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
    run_case_bf3(L, H, B, T)         # a fresh engine after the time-out: correct results
    ops.lstm_bidir_fwd(ws, ks, bs, dlen)
    ops.lstm_bidir_bwd(ws, ks, dks, dbs, dlen)
    torch.cuda.synchronize()
    ops.lstm_bidir_status(ws)


def test_bf3_plain_bf16_stays_refused():
    from rnn_speech_amd.engine import Engine
    with pytest.raises(ValueError, match="f32"):
        Engine(2, 64, 20, 80, 3, 10, 4, bidirectional=True, bidirectional_mode="layer", precision="bf16")
    eng = Engine(2, 64, 20, 80, 3, 10, 4, bidirectional=True, bidirectional_mode="layer", precision="bf16x3")
    assert eng.lstm_ws.desc.precision == 1


def test_bf3_engine_training_loss_falls_and_state_round_trips():
    L, H, D, C, B, T, U = 2, 64, 20, 30, 8, 30, 6
    eng, p = base.make_engine(L, H, D, C, B, T, U, precision="bf16x3")
    x, lengths, dense = base.make_batch(T, B, D, C, U, seed=12)
    dx, dlen, dlab = torch.as_tensor(x).cuda(), torch.as_tensor(lengths).cuda(), torch.as_tensor(dense).cuda()
    losses = []
    for _ in range(20):
        eng.zero_grads()
        losses.append(float(eng.mini_batch(dx, dlen, dlab).sum()))
        eng.apply(3e-3, 5.0)
    torch.cuda.synchronize()
    eng.check()
    assert eng.kernel_path()["layer_product"] == "bf16x3"
    assert losses[-1] < 0.7 * losses[0], losses
    snap = eng.to_numpy()
    eng2, _ = base.make_engine(L, H, D, C, B, T, U, seed=1, precision="bf16x3")
    eng2.load_numpy(snap)
    a = eng.forward(dx, dlen).clone()
    b = eng2.forward(dx, dlen).clone()
    torch.cuda.synchronize()
    assert torch.equal(a, b)


def _synth(seed, n, sr=16000):
    rng = np.random.RandomState(seed)
    t = np.arange(n) / float(sr)
    return (0.1 * rng.randn(n) + 0.3 * np.sin(2 * np.pi * 300 * (1 + seed % 5) * t)).astype(np.float32)


def test_bf3_drop_in_train_step_from_config(tmp_path):
    """precision : bf16x3 with bidirectional : True, bidirectional_mode : layer in config.ini reaches the engine the way stt.py
    builds its model, and one run_train_step trains."""
    from util.hyperparams import read_config_file
    from models.AcousticModel import AcousticModel, Session
    from models.SpeechRecognizer import SpeechRecognizer
    src = open(os.path.join(ROOT, "config.ini")).read()
    src = src.replace("checkpoint_dir", "checkpoint_dir : %s\n#" % (tmp_path / "ckpt"), 1)
    src = src.replace("precision : f32", "precision : bf16x3", 1).replace("bidirectional : False", "bidirectional : True", 1)
    src = src.replace("[acoustic_network_params]", "[acoustic_network_params]\nbidirectional_mode : layer", 1)
    cfg = tmp_path / "config.ini"
    cfg.write_text(src)
    hp = read_config_file(str(cfg))
    assert (hp["precision"], hp["bidirectional"], hp["bidirectional_mode"]) == ("bf16x3", True, "layer")
    cm = SpeechRecognizer("english").get_char_map()
    T, U, B = 60, 12, 2
    items = [[(_synth(i, 16000 // 2 + 37 * i), 16000), txt, None] for i, txt in enumerate(["hello there", "it'll do", "good bye"])]
    model = AcousticModel(2, 64, B, T, U, 20, False, len(cm))
    model.precision = hp["precision"]
    model.bidirectional = hp["bidirectional"]
    model.bidirectional_mode = hp["bidirectional_mode"]
    sess = Session()
    t_it, v_it = model.add_datasets_input(model.build_dataset(items, B, T, U, "mfcc", cm),
                                          model.build_dataset(items[:2], B, T, U, "mfcc", cm))
    sess.run(t_it.initializer)
    sess.run(v_it.initializer)
    model.create_training_rnn(hp["dropout_input_keep_prob"], hp["dropout_output_keep_prob"], 1, 1e-3, 0.33, use_iterator=True)
    model.initialize(sess)
    eng = model.engine
    assert eng.layerwise and eng.precision == "bf16x3"
    before = eng.params.clone()
    loss, err, step, empty = model.run_train_step(sess, 1, 1.0)
    assert step == 1 and not empty and np.isfinite(loss)
    assert eng.kernel_path()["layer_product"] == "bf16x3"
    assert not torch.equal(before, eng.params)
