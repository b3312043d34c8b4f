"""ms per optimiser step with SpecAugment off and on at the headline shape: 3 x 512, 40-dim MFCC, batch 32, 1001 frames of 16 kHz
audio, exact f32, dropout keep 0.8 / 0.5, PCM and labels resident in HBM.  A step is front end -> (masks) -> forward, CTC, backward
-> clip + Adam, on one stream, no input pipelining.  Policy: 2 frequency masks of up to 7 bins, 2 time masks of up to 40 frames, no
time mask above 0.2 of its utterance.  The two settings alternate in one process on ONE engine: a window of --steps steps off, then
one on; median of --windows windows after --warmup windows.  One JSON line.  A measurement, not a gate.

    python tools/spec_augment_bench.py [--steps 10] [--windows 5] [--warmup 3]

The kernel's own time per launch comes from a separate run under the profiler, which serialises kernels and so says nothing about
the step:

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/spec_augment_bench.py --mask-only 200

--mask-only N: the front end once, then N masking launches alone, each with another seed (read spec_augment_kernel's average in
OUT's kernel_stats.csv).
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
POLICY = dict(period=D, freq_masks=2, freq_width=7, time_masks=2, time_width=40, time_permille=200)


def synth_pcm(seed, n):
    rng = np.random.RandomState(seed)
    t = np.arange(n) / float(SR)
    sig = 0.1 * rng.randn(n)
    for f0, a in ((220.0, 0.3), (1330.0, 0.2), (3100.0, 0.1)):
        sig += a * np.sin(2 * np.pi * f0 * (1 + 0.01 * (seed % 17)) * t)
    return sig.astype(np.float32)


def synth_labels(rng):
    """80 .. 160 tokens and an EOS per utterance, as bench.py draws them."""
    dense = np.zeros((B, U), np.int32)
    for b in range(B):
        n = rng.randint(80, 161)
        dense[b, :n - 1] = rng.randint(1, C - 1, size=n - 1)
        dense[b, n - 1] = C - 1
    return dense


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--mask-only", type=int, default=0)
    a = ap.parse_args()
    from rnn_speech_amd import ops
    from rnn_speech_amd.engine import Engine

    n = SR * SECONDS
    pcm = torch.from_numpy(np.stack([synth_pcm(b, n) for b in range(B)])).cuda()
    n_samples = [n] * B
    plan = ops.spec_augment_plan(T, B, D, POLICY)
    feat, nf = ops.frontend(pcm, n_samples, SR, "mfcc", T, D)
    lengths = torch.tensor([min(f, T) for f in nf], dtype=torch.int32).cuda()      # resident, like the PCM and the labels

    if a.mask_only:
        for i in range(a.mask_only):
            ops.spec_augment(feat, lengths, POLICY, (7 << 32) | ((i + 1) * 0x9E3779B1 & 0xFFFFFFFF))
        torch.cuda.synchronize()
        zeros = int((feat == 0).sum())
        print(json.dumps({"mask_only_launches": a.mask_only, "plan": plan, "zero_words_at_the_end": zeros, "words": feat.numel()}))
        return

    dlab = torch.from_numpy(synth_labels(np.random.RandomState(100))).cuda()
    eng = Engine(L, H, D, C, B, T, U, seed=1234)
    torch.cuda.synchronize()
    torch.cuda.set_stream(eng.stream)          # a real (non-NULL) stream for the whole job (Engine.on_stream)
    masked_words = []

    def step(on, i):
        feat, _ = ops.frontend(pcm, n_samples, SR, "mfcc", T, D)
        if on:
            ops.spec_augment(feat, lengths, POLICY, (7 << 32) | ((i + 1) * 0x9E3779B1 & 0xFFFFFFFF))
        eng.zero_grads()
        eng.mini_batch(feat, lengths, dlab, 0.8, 0.5, seed=i + 1)
        eng.apply(3e-4, 1.0)
        return feat

    def window(on, w):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for i in range(a.steps):
            feat = step(on, w * a.steps + i)
        t1.record()
        t1.synchronize()
        if on:
            masked_words.append(int((feat == 0).sum()))
        return t0.elapsed_time(t1) / a.steps

    ms = {"off": [], "on": []}
    for w in range(a.warmup + a.windows):
        for key in ms:
            t = window(key == "on", w)
            if w >= a.warmup:
                ms[key].append(t)
    eng.check()
    loss = eng.loss.cpu().numpy()
    assert np.isfinite(loss).all() and (loss > 0).all()
    out = {"shape": "%dx%d, %d-dim mfcc, batch %d, %d frames, f32, dropout 0.8/0.5" % (L, H, D, B, T), "policy": POLICY,
           "ms_per_step": {k: float(np.median(v)) for k, v in ms.items()},
           "ms_per_step_min_max": {k: [float(np.min(v)), float(np.max(v))] for k, v in ms.items()},
           "ratio": float(np.median(ms["on"]) / np.median(ms["off"])), "masked_words_last_step": masked_words[-1],
           "words": T * B * D, "steps_per_window": a.steps, "windows": a.windows, "warmup_windows": a.warmup,
           "spec_augment_plan": plan}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
