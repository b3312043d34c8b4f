"""ms per optimiser step with speed perturbation off and on at the headline shape: 3 x 512, 40-dim MFCC, batch 32, 10 s of 16 kHz PCM
per row resident in HBM, t_max 1001, exact f32, dropout keep 0.8 / 0.5.  A step is (per-row resampling) -> front end -> forward, CTC,
backward -> clip + Adam, on one stream, no input pipelining.  Factors 0.9 / 1.0 / 1.1, one drawn per row and step
(ops.speed_perturb_draw); a row at 0.9 grows to 11.1 s and is truncated at t_max by the front end, as any over-long file is.  The two
settings alternate in one process on ONE engine: a window of --steps steps off, then one on; median of --windows windows after
--warmup windows.  One JSON line.  A measurement, not a gate: resampling is real added work.

    python tools/speed_perturb_bench.py [--steps 10] [--windows 5] [--warmup 3]

The kernels' own times per launch come from a separate run under the profiler, which serialises kernels and so says nothing about
the step:

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/speed_perturb_bench.py --resample-only 50

--resample-only N, in ONE process: N launches (after 5 warm-up launches each) of ops.resample_rows at 1000 permille (what
ops.resample runs) and at mixed 900 / 1000 / 1100, in that order, on B 32 rows of 10 s of audio; --rates IN OUT sets the two rates
(default 16,000 -> 22,050).  Without the profiler the JSON line's ms_per_call holds the two whole-call times (table, length and
resampling launches) between device events.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

L, H, D, C, B, T, U = 3, 512, 40, 80, 32, 1001, 161
SR, SECONDS, LOAD_SR = 16000, 10, 22050
FACTORS = [900, 1000, 1100]
SEED = 7 << 32


def synth_pcm(seed, n, rate=SR):
    rng = np.random.RandomState(seed)
    t = np.arange(n) / float(rate)
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
    ap.add_argument("--resample-only", type=int, default=0)
    ap.add_argument("--rates", type=int, nargs=2, metavar=("IN", "OUT"), default=[SR, LOAD_SR])
    a = ap.parse_args()
    from rnn_speech_amd import ops
    from rnn_speech_amd.engine import Engine

    rate_in, rate_out = a.rates if a.resample_only else (SR, SR)
    n = rate_in * SECONDS
    pcm = torch.from_numpy(np.stack([synth_pcm(b, n, rate_in) for b in range(B)])).cuda()
    n_samples = [n] * B
    mixed = [FACTORS[b % 3] for b in range(B)]

    if a.resample_only:
        plans = {"uniform_1000": ops.resample_rows_plan(n_samples, [1000] * B, n, rate_in, rate_out),
                 "mixed_900_1000_1100": ops.resample_rows_plan(n_samples, mixed, n, rate_in, rate_out)}

        def timed(fn):
            """ms per whole call (table, length and resampling launches) between device events, after 5 warm-up calls."""
            for _ in range(5):
                fn()
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(a.resample_only):
                out = fn()
            t1.record()
            t1.synchronize()
            return out, t0.elapsed_time(t1) / a.resample_only

        (_, n_new), ms_new = timed(lambda: ops.resample_rows(pcm, n_samples, [1000] * B, rate_in, rate_out))
        (_, n_mix), ms_mix = timed(lambda: ops.resample_rows(pcm, n_samples, mixed, rate_in, rate_out))
        torch.cuda.synchronize()
        print(json.dumps({"resample_only_launches": a.resample_only, "rates": [rate_in, rate_out], "rows": B, "samples_in": n,
                          "samples_out": n_new[0], "samples_out_mixed": sorted(set(n_mix)),
                          "ms_per_call": {"resample_rows_1000": ms_new, "resample_rows_mixed": ms_mix},
                          "plans": plans}))
        return

    plan = ops.resample_rows_plan(n_samples, mixed, n, SR, SR)
    feat, nf = ops.frontend(pcm, n_samples, SR, "mfcc", T, D)
    lengths_off = torch.tensor([min(f, T) for f in nf], dtype=torch.int32)
    dlab = torch.from_numpy(synth_labels(np.random.RandomState(100))).cuda()
    eng = Engine(L, H, D, C, B, T, U, seed=1234)
    torch.cuda.synchronize()
    torch.cuda.set_stream(eng.stream)          # a real (non-NULL) stream for the whole job (Engine.on_stream)
    frames_on = []

    def step(on, i):
        if on:
            speeds = [ops.speed_perturb_draw(SEED, (i << 32) | b, FACTORS) for b in range(B)]
            x, n_x = ops.resample_rows(pcm, n_samples, speeds, SR, SR)
            feat, nf = ops.frontend(x, n_x, SR, "mfcc", T, D)
            lengths = torch.tensor([min(f, T) for f in nf], dtype=torch.int32).cuda()
            frames_on.append(int(sum(min(f, T) for f in nf)))
        else:
            feat, nf = ops.frontend(pcm, n_samples, SR, "mfcc", T, D)
            lengths = torch.tensor([min(f, T) for f in nf], dtype=torch.int32).cuda()      # (the same small copy in both settings)
        eng.zero_grads()
        eng.mini_batch(feat, lengths, dlab, 0.8, 0.5, seed=i + 1)
        eng.apply(3e-4, 1.0)

    def window(on, w):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for i in range(a.steps):
            step(on, w * a.steps + i)
        t1.record()
        t1.synchronize()
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
    out = {"shape": "%dx%d, %d-dim mfcc, batch %d, %d s of %d Hz PCM, t_max %d, f32, dropout 0.8/0.5" % (L, H, D, B, SECONDS, SR, T),
           "factors_permille": FACTORS,
           "ms_per_step": {k: float(np.median(v)) for k, v in ms.items()},
           "ms_per_step_min_max": {k: [float(np.min(v)), float(np.max(v))] for k, v in ms.items()},
           "ratio": float(np.median(ms["on"]) / np.median(ms["off"])),
           "frames_per_step": {"off": int(lengths_off.sum()), "on_mean": float(np.mean(frames_on))},
           "steps_per_window": a.steps, "windows": a.windows, "warmup_windows": a.warmup, "resample_rows_plan": plan}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
