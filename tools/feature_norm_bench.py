"""ms per optimiser step with feature normalisation off and on at the headline shape: 3 x 512, 40-dim MFCC, batch 32, 1001 frames of
16 kHz audio, exact f32, dropout keep 0.8 / 0.5, PCM and labels resident in HBM.  A step is front end -> (normalisation) -> forward,
CTC, backward -> clip + Adam, on one stream, no input pipelining.  The settings alternate in one process on ONE engine: a window of
--steps steps off, then one in utterance mode, then one in global mode; median of --windows windows after --warmup windows.  One JSON
line.  A measurement, not a gate.

    python tools/feature_norm_bench.py [--steps 10] [--windows 5] [--warmup 3]

The kernels' own time per launch comes from a separate run under the profiler, which serialises kernels and so says nothing about
the step:

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/feature_norm_bench.py --norm-only 200

--norm-only N: the front end once, then N utterance-mode calls (feature_moments_kernel + feature_norm_apply_kernel) and N global-mode
calls (feature_norm_apply_kernel from a table) alone, each on a fresh copy of the features (read the kernels' averages in OUT's
kernel_stats.csv; the utterance-mode and the global-mode apply kernels are two instantiations and are listed apart).
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
MODES = ("off", "utterance", "global")


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
    ap.add_argument("--norm-only", type=int, default=0)
    a = ap.parse_args()
    from rnn_speech_amd import ops
    from rnn_speech_amd.engine import Engine
    from rnn_speech_amd.feature_norm import FeatureStats, describe

    n = SR * SECONDS
    pcm = torch.from_numpy(np.stack([synth_pcm(b, n) for b in range(B)])).cuda()
    n_samples = [n] * B
    plans = {mode: ops.feature_norm_plan(B, D, T, mode) for mode in ("utterance", "global")}
    feat, nf = ops.frontend(pcm, n_samples, SR, "mfcc", T, D)
    lengths = torch.tensor([min(f, T) for f in nf], dtype=torch.int32).cuda()      # resident, like the PCM and the labels
    table = FeatureStats(describe("mfcc", D, SR, D)).accumulate(feat, nf).table()

    def normalise(x, mode):
        if mode != "off":
            ops.feature_norm(x, nf, mode, table=table if mode == "global" else None)
        return x

    if a.norm_only:
        for mode in ("utterance", "global"):
            for _ in range(a.norm_only):
                out = normalise(feat.clone(), mode)
        torch.cuda.synchronize()
        c0 = feat[:, :, 0].double()
        print(json.dumps({"norm_only_calls_per_mode": a.norm_only, "plans": plans, "c0_mean_before": float(c0.mean()),
                          "c0_mean_after_global": float(out[:, :, 0].double().mean())}))
        return

    dlab = torch.from_numpy(synth_labels(np.random.RandomState(100))).cuda()
    eng = Engine(L, H, D, C, B, T, U, seed=1234)
    torch.cuda.synchronize()
    torch.cuda.set_stream(eng.stream)          # a real (non-NULL) stream for the whole job (Engine.on_stream)

    def step(mode, i):
        x, _ = ops.frontend(pcm, n_samples, SR, "mfcc", T, D)
        normalise(x, mode)
        eng.zero_grads()
        eng.mini_batch(x, lengths, dlab, 0.8, 0.5, seed=i + 1)
        eng.apply(3e-4, 1.0)

    def window(mode, w):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for i in range(a.steps):
            step(mode, w * a.steps + i)
        t1.record()
        t1.synchronize()
        return t0.elapsed_time(t1) / a.steps

    ms = {mode: [] for mode in MODES}
    for w in range(a.warmup + a.windows):
        for mode in MODES:
            t = window(mode, w)
            if w >= a.warmup:
                ms[mode].append(t)
    eng.check()
    loss = eng.loss.cpu().numpy()
    assert np.isfinite(loss).all() and (loss > 0).all()
    med = {k: float(np.median(v)) for k, v in ms.items()}
    out = {"shape": "%dx%d, %d-dim mfcc, batch %d, %d frames, f32, dropout 0.8/0.5" % (L, H, D, B, T),
           "ms_per_step": med, "ms_per_step_min_max": {k: [float(np.min(v)), float(np.max(v))] for k, v in ms.items()},
           "ratio": {k: med[k] / med["off"] for k in MODES[1:]}, "steps_per_window": a.steps, "windows": a.windows,
           "warmup_windows": a.warmup, "feature_norm_plans": plans}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
