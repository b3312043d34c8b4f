"""ms per optimiser step with and without low frame rate input (frame_stack / frame_skip) at the headline shape: 3 x 512, 40-dim
MFCC, batch 32, 1001 source frames of 16 kHz audio, exact f32, dropout keep 0.8 / 0.5, PCM and labels resident in HBM.  A step is
front end -> (frame stacking) -> forward, CTC, backward -> clip + Adam, on one stream, no input pipelining.  The two settings
alternate in one process: a window of --steps steps at (1, 1), then one at (--stack, --skip); median of --windows windows after
--warmup windows.  One JSON line.  A measurement, not a gate.

    python tools/lfr_bench.py [--stack 3] [--skip 3] [--steps 10] [--windows 5] [--warmup 3]

The kernel's own time per launch comes from a separate run under the profiler, which serialises kernels and so says nothing about
the step:

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/lfr_bench.py --stack-only 200

--stack-only N: the front end once, then N frame stacking launches alone (read frame_stack_kernel's average in OUT's kernel_stats.csv).
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

L, H, D, C, B, T, U = 3, 512, 40, 80, 32, 1001, 161
SR, SECONDS = 16000, 10


def synth_pcm(seed, n):
    rng = np.random.RandomState(seed)
    t = np.arange(n) / float(SR)
    sig = 0.1 * rng.randn(n)
    for f0, a in ((220.0, 0.3), (1330.0, 0.2), (3100.0, 0.1)):
        sig += a * np.sin(2 * np.pi * f0 * (1 + 0.01 * (seed % 17)) * t)
    return sig.astype(np.float32)


def synth_labels(rng, t_model):
    """80 .. 160 tokens and an EOS per utterance, as bench.py draws them; never more than a third of the model's frames, so that
    every row keeps a feasible alignment at every setting."""
    dense = np.zeros((B, U), np.int32)
    for b in range(B):
        n = min(rng.randint(80, 161), t_model // 3)
        dense[b, :n - 1] = rng.randint(1, C - 1, size=n - 1)
        dense[b, n - 1] = C - 1
    return dense


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--stack", type=int, default=3)
    ap.add_argument("--skip", type=int, default=3)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--stack-only", type=int, default=0)
    a = ap.parse_args()
    from rnn_speech_amd import ops
    from rnn_speech_amd.engine import Engine

    n = SR * SECONDS
    pcm = torch.from_numpy(np.stack([synth_pcm(b, n) for b in range(B)])).cuda()
    n_samples = [n] * B
    plan = ops.frame_stack_plan(B, D, T, a.stack, a.skip)
    t_model = plan["t_out"]

    if a.stack_only:
        feat, nf = ops.frontend(pcm, n_samples, SR, "mfcc", T, D)
        out = torch.empty(t_model, B, plan["d_out"], device="cuda")
        for _ in range(a.stack_only):
            ops.frame_stack(feat, nf, a.stack, a.skip, out=out)
        torch.cuda.synchronize()
        print(json.dumps({"stack_only_launches": a.stack_only, "plan": plan}))
        return

    dlab = torch.from_numpy(synth_labels(np.random.RandomState(100), t_model)).cuda()      # the same targets at both settings
    settings = {"1x1": (1, 1, Engine(L, H, D, C, B, T, U, seed=1234)),
                "%dx%d" % (a.stack, a.skip): (a.stack, a.skip, Engine(L, H, plan["d_out"], C, B, t_model, U, seed=1234))}
    torch.cuda.synchronize()
    torch.cuda.set_stream(settings["1x1"][2].stream)          # a real (non-NULL) stream for the whole job (Engine.on_stream)
    losses, lengths_dev = {}, {}

    def step(key, i):
        k, s, eng = settings[key]
        feat, nf = ops.frontend(pcm, n_samples, SR, "mfcc", T, D)
        if (k, s) != (1, 1):
            feat, nf = ops.frame_stack(feat, nf, k, s)
        if key not in lengths_dev:          # (the same every step: resident, like the PCM and the labels)
            lengths_dev[key] = torch.tensor([min(f, eng.T) for f in nf], dtype=torch.int32).cuda()
        lengths = lengths_dev[key]
        eng.zero_grads()
        eng.mini_batch(feat, lengths, dlab, 0.8, 0.5, seed=i + 1)
        eng.apply(3e-4, 1.0)
        losses[key] = eng.loss

    def window(key, w):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for i in range(a.steps):
            step(key, w * a.steps + i)
        t1.record()
        t1.synchronize()
        return t0.elapsed_time(t1) / a.steps

    ms = {key: [] for key in settings}
    for w in range(a.warmup + a.windows):
        for key in settings:
            t = window(key, w)
            if w >= a.warmup:
                ms[key].append(t)
    for key, (_, _, eng) in settings.items():
        eng.check()
        assert np.isfinite(losses[key].cpu().numpy()).all() and (losses[key].cpu().numpy() > 0).all(), key
    base, lfr = [k for k in settings]
    out = {"shape": "%dx%d, %d-dim mfcc, batch %d, %d source frames, f32, dropout 0.8/0.5" % (L, H, D, B, T),
           "model_frames": {base: T, lfr: t_model}, "input_dim": {base: D, lfr: plan["d_out"]},
           "ms_per_step": {k: float(np.median(v)) for k, v in ms.items()},
           "ms_per_step_min_max": {k: [float(np.min(v)), float(np.max(v))] for k, v in ms.items()},
           "ratio": float(np.median(ms[lfr]) / np.median(ms[base])), "steps_per_window": a.steps, "windows": a.windows,
           "warmup_windows": a.warmup, "frame_stack_plan": plan}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
