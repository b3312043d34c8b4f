"""The language-model step at 2 x 512, V 80, batch 64, rows of 161 predicted positions (160 tokens and the closing EOS), exact f32,
dropout keep 0.9 / 0.9: ms per optimiser step (embed_fwd -> lstm_fwd -> output Linear -> xent_fwd_bwd -> output Linear backward ->
lstm_bwd -> embed_bwd -> clip + Adam) on one stream, tokens resident in HBM; and, in the same process, the two new ends against
what could be done before them:

  embed_fwd + embed_bwd   against a materialised one-hot [T*B, V] through linear_fwd / linear_bwd (the reference's own graph);
  xent_fwd_bwd            against torch's log_softmax + nll_loss forward and backward on the same tensors.

Synthetic and seeded: token ids drawn with the skew of text (one token holds about a fifth of all positions), row lengths 81 .. 161.
Each pair alternates in windows of --reps calls; median of --windows windows after --warmup windows.  One JSON line.  A
measurement, not a gate.

    python tools/lm_bench.py [--steps 10] [--reps 50] [--windows 5] [--warmup 2]

Kernel times come from a separate run under the profiler, which serialises kernels and so says nothing about the step:

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/lm_bench.py --steps-only 20
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

L, H, V, B, T = 2, 512, 80, 64, 161


def synth_tokens(seed):
    """tok int32 [B, T + 1] = [V-1, y.., V-1] padded with V-1, lengths int32 [B] in 81 .. 161; token 0 takes a fifth of the draws."""
    rng = np.random.RandomState(seed)
    p = np.full(V - 1, 0.8 / (V - 2))
    p[0] = 0.2
    tok = np.full((B, T + 1), V - 1, np.int32)
    lengths = rng.randint(81, T + 1, size=B).astype(np.int32)
    lengths[0] = T
    for b in range(B):
        tok[b, 1:lengths[b]] = rng.choice(V - 1, size=lengths[b] - 1, p=p)
    return tok, lengths


def timed(fn, reps):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        fn()
    t1.record()
    t1.synchronize()
    return 1e3 * t0.elapsed_time(t1) / reps          # microseconds per call


def alternate(pair, reps, windows, warmup):
    us = {k: [] for k in pair}
    for w in range(warmup + windows):
        for k, fn in pair.items():
            t = timed(fn, reps)
            if w >= warmup:
                us[k].append(t)
    return {k: float(np.median(v)) for k, v in us.items()}, {k: [float(np.min(v)), float(np.max(v))] for k, v in us.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--steps-only", type=int, default=0)
    a = ap.parse_args()
    from rnn_speech_amd import ops
    from rnn_speech_amd.language_model import LmEngine

    tok_h, len_h = synth_tokens(1)
    tok, lengths = torch.from_numpy(tok_h).cuda(), torch.from_numpy(len_h).cuda()
    n_tok = int(len_h.sum())
    eng = LmEngine(L, H, V, B, T, seed=1234)
    stream = torch.cuda.Stream(priority=-1)
    torch.cuda.synchronize()
    torch.cuda.set_stream(stream)              # a real (non-NULL) stream for the whole job, as Engine.on_stream gives the acoustic step

    def step(i=[0]):
        i[0] += 1
        eng.zero_grads()
        eng.mini_batch(tok, lengths, 0.9, 0.9, seed=i[0], max_len=T, scale=1.0 / n_tok)
        eng.apply(1e-3, 5.0)

    if a.steps_only:
        for _ in range(a.steps_only):
            step()
        torch.cuda.synchronize()
        eng.check()
        print(json.dumps({"steps_only": a.steps_only, "path": eng.kernel_path(), "xent_plan": ops.xent_plan(T, B, V),
                          "mean_token_nll": float(eng.loss.sum().cpu()) / n_tok}))
        return

    step_us, step_span = alternate({"lm_step": step}, a.steps, a.windows, a.warmup)
    eng.check()
    loss = eng.loss.cpu().numpy()
    assert np.isfinite(loss).all() and (loss[len_h > 0] > 0).all()

    # ---- the token lookup and its backward against the one-hot products
    w, bias = eng.p("input_w"), eng.p("input_b")
    z = torch.empty(T, B, H, device="cuda")
    dz = torch.randn(T, B, H, device="cuda", generator=torch.Generator(device="cuda").manual_seed(2))
    dw, db = torch.zeros(V, H, device="cuda"), torch.zeros(H, device="cuda")
    live = (np.arange(T)[:, None] < len_h[None, :])
    onehot_h = np.zeros((T, B, V), np.float32)
    tt, bb = np.nonzero(live)
    onehot_h[tt, bb, tok_h[bb, tt]] = 1.0
    onehot = torch.from_numpy(onehot_h).cuda().view(T * B, V)

    def embed():
        ops.embed_fwd(tok, lengths, w, bias, z)
        ops.embed_bwd(tok, lengths, dz, dw, db)

    def onehot_linear():
        ops.linear_fwd(onehot, w, bias, out=z.view(T * B, H))
        ops.linear_bwd(onehot, w, dz.view(T * B, H), dw, db, need_dx=False)

    embed_us, embed_span = alternate({"embed_fwd_bwd": embed, "onehot_linear_fwd_bwd": onehot_linear}, a.reps, a.windows, a.warmup)

    # ---- the cross-entropy against torch's log_softmax + nll_loss, forward and backward
    logits = torch.randn(T, B, V, device="cuda", generator=torch.Generator(device="cuda").manual_seed(3))
    dlogits, nll, loss_b = torch.empty_like(logits), torch.empty(T, B, device="cuda"), torch.empty(B, device="cuda")
    targets = tok[:, 1:]
    tgt_long = torch.from_numpy(np.where(live, tok_h[:, 1:].T, -100).astype(np.int64)).cuda().view(T * B)
    leaf = logits.clone().requires_grad_(True)

    def xent():
        ops.xent_fwd_bwd(logits, targets, lengths, scale=1.0 / n_tok, nll=nll, loss=loss_b, dlogits=dlogits)

    def torch_xent():
        leaf.grad = None
        out = torch.nn.functional.nll_loss(torch.log_softmax(leaf.view(T * B, V), dim=1), tgt_long, ignore_index=-100, reduction="sum")
        (out / n_tok).backward()

    xent_us, xent_span = alternate({"xent_fwd_bwd": xent, "torch_log_softmax_nll_fwd_bwd": torch_xent}, a.reps, a.windows, a.warmup)
    worst = float((dlogits - leaf.grad).abs().max().cpu())
    traffic = 2 * T * B * V * 4
    out = {"shape": "%dx%d, V %d, batch %d, rows of %d, f32, dropout 0.9/0.9" % (L, H, V, B, T), "tokens_per_step": n_tok,
           "lstm_path": eng.kernel_path(), "xent_plan": ops.xent_plan(T, B, V),
           "us_per_step": step_us["lm_step"], "us_per_step_min_max": step_span["lm_step"],
           "embed_us": embed_us, "embed_us_min_max": embed_span, "xent_us": xent_us, "xent_us_min_max": xent_span,
           "xent_bytes": traffic, "xent_gb_per_s": traffic / xent_us["xent_fwd_bwd"] * 1e-3,
           "xent_max_abs_diff_to_torch": worst, "steps_per_window": a.steps, "reps_per_window": a.reps, "windows": a.windows,
           "warmup_windows": a.warmup}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
