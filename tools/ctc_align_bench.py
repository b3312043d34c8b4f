"""ms per call of the CTC aligner (ops.ctc_align: log-softmax, Viterbi recursion, walk back) beside the CTC loss + gradient
(ops.ctc_loss_fwd_bwd: log-softmax, alpha and beta recursions, gradient) at the same shape in the same process, the two calls
alternating.  Median of --steps after --warmup, device events around each call; random logits, every utterance full length, all U
label slots used.  One JSON line per shape.

    python tools/ctc_align_bench.py [--steps 5] [--warmup 2] [--calls 10]

--calls: calls queued back to back inside one timed window (the figure is the window over their number: a single call of a few
hundred microseconds would measure the launch path as much as the kernels).
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = [(32, 1001, 63), (32, 1001, 161), (32, 1001, 255), (32, 1001, 511), (32, 1300, 1100), (10, 3510, 600)]      # B, T, U


def timed(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls


def run(B, T, U, steps, warmup, calls, C=80):
    from rnn_speech_amd import ops
    rng = np.random.RandomState(T + U)
    logits = torch.as_tensor((rng.randn(T, B, C) * 2).astype(np.float32)).cuda()
    lab = rng.randint(1, C - 1, size=(B, U))      # (a repeat every ~C labels: T frames suffice at every shape)
    dense = torch.as_tensor(lab.astype(np.int32)).cuda()
    lengths = torch.full((B,), T, dtype=torch.int32).cuda()
    aws = ops.CtcAlignWorkspace(T, B, C, U)
    lws = ops.CtcWorkspace(T, B, C, U)
    loss = torch.empty(B, device="cuda")
    dlogits = torch.empty_like(logits)
    out = {}
    align = lambda: out.__setitem__("al", ops.ctc_align(logits, dense, lengths, ws=aws))
    lossf = lambda: ops.ctc_loss_fwd_bwd(logits, dense, lengths, ws=lws, loss=loss, dlogits=dlogits)
    ta, tl = [], []
    for i in range(warmup + steps):
        x, y = timed(align, calls), timed(lossf, calls)
        if i >= warmup:
            ta.append(x)
            tl.append(y)
    score = out["al"].score.cpu().numpy()
    assert np.isfinite(score).all() and np.isfinite(loss.cpu().numpy()).all() and (score <= -loss.cpu().numpy() + 1e-3).all()
    return {"B": B, "T": T, "U": U, "align_kernel": "%(kernel)s/%(rmax)d" % ops.ctc_align_plan(T, B, C, U),
            "loss_kernel": "%(kernel)s/%(rmax)d" % ops.ctc_plan(T, B, C, U), "align_ms": float(np.median(ta)), "loss_fwd_bwd_ms": float(np.median(tl)),
            "align_ms_min": float(np.min(ta)), "loss_fwd_bwd_ms_min": float(np.min(tl)), "steps": steps, "calls_per_window": calls,
            "align_workspace_mb": aws.buf.numel() / 2.0 ** 20}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--calls", type=int, default=10)
    a = ap.parse_args()
    for B, T, U in SHAPES:
        print(json.dumps(run(B, T, U, a.steps, a.warmup, a.calls)), flush=True)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
