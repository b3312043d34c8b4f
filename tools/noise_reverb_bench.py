"""Noise and reverberation augmentation: the three launches on their own, and the headline step with and without the stage.

    python tools/noise_reverb_bench.py [--steps 10] [--windows 5] [--warmup 3] [--taps 4096]

ms per optimiser step at the headline shape (3 x 512, 40-dim MFCC, batch 32, 10 s of 16 kHz PCM per row resident in HBM, t_max 1001,
exact f32, dropout keep 0.8 / 0.5) with the input pipelined as bench.py pipelines it: the pre-processing of step k + 1 runs on a side
stream beside the forward recurrence of step k.  "off": front end only.  "on": ops.reverb_rows (every row, --taps taps) ->
ops.row_sumsq -> ops.noise_mix_rows (every row, SNR drawn per row and step, ops.augment_draw at probability 1) -> front end.  The two
settings alternate in one process on ONE engine: a window of --steps steps off, then one on; median of --windows windows after
--warmup windows.  One JSON line.  A measurement, not a gate.

The kernels' own times per launch come from a separate run under the profiler, which serialises kernels and so says nothing about
the step:

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/noise_reverb_bench.py --launches 20

--launches N, in ONE process: N launches (after 3 warm-up launches each) of ops.reverb_rows with 1024-, 4096- and 8192-tap impulse
responses, of ops.row_sumsq and of ops.noise_mix_rows (in place), in that order, on B 32 rows of 10 s of 22.05 kHz audio.  Without
the profiler the JSON line's ms_per_call holds the whole-call times (row-value and kernel launches) between device events, the
reverberation's algorithmic rate 2 L n B / time and the two bandwidth-bound launches' bytes / time.
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
SEED = 9 << 32
SNR = (50, 200)
F32_PEAK_TF = 157.3


def synth_pcm(seed, n, rate=SR):
    rng = np.random.RandomState(seed)
    t = np.arange(n) / float(rate)
    sig = 0.1 * rng.randn(n)
    for f0, a in ((220.0, 0.3), (1330.0, 0.2), (3100.0, 0.1)):
        sig += a * np.sin(2 * np.pi * f0 * (1 + 0.01 * (seed % 17)) * t)
    return sig.astype(np.float32)


def synth_rir(taps, seed):
    """Exponentially decaying noise behind a direct path at sample 64, unit energy."""
    rng = np.random.RandomState(500 + seed)
    h = 0.2 * rng.randn(taps) * np.exp(-np.arange(taps) / (taps / 5.0))
    h[:min(64, taps - 1)] = 0.0
    h[min(64, taps - 1)] = 1.0
    return (h / np.sqrt(np.sum(h * h))).astype(np.float32)


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
    ap.add_argument("--taps", type=int, default=4096)
    ap.add_argument("--launches", type=int, default=0)
    a = ap.parse_args()
    from rnn_speech_amd import ops
    from rnn_speech_amd.audioprocessor import AugmentBank
    from rnn_speech_amd.engine import Engine

    if a.launches:
        n = LOAD_SR * SECONDS
        pcm = torch.from_numpy(np.stack([synth_pcm(b, n, LOAD_SR) for b in range(B)])).cuda()
        n_samples = [n] * B
        noises = [synth_pcm(100 + m, LOAD_SR * (3 + 2 * m), LOAD_SR) * 0.2 for m in range(4)]

        def timed(fn):
            """ms per whole call between device events, after 3 warm-up calls."""
            for _ in range(3):
                fn()
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(a.launches):
                fn()
            t1.record()
            t1.synchronize()
            return t0.elapsed_time(t1) / a.launches

        ms, plans, rate = {}, {}, {}
        out = torch.empty_like(pcm)
        for taps in (1024, 4096, 8192):
            bank = AugmentBank([synth_rir(taps, r) for r in range(4)], noises)
            idx = [b % 4 for b in range(B)]
            key = "reverb_rows_%d" % taps
            plans[key] = ops.reverb_rows_plan(n_samples, n, bank.rir_taps, bank.rir_delay, taps, idx)
            ms[key] = timed(lambda: ops.reverb_rows(pcm, n_samples, bank.rir_bank, bank.rir_taps, bank.rir_delay, idx, out=out))
            tf = 2.0 * taps * n * B / (ms[key] * 1e-3) / 1e12
            rate[key] = {"algorithmic_tflops": tf, "fraction_of_f32_peak": tf / F32_PEAK_TF}
        energy = torch.empty(B, device="cuda", dtype=torch.float64)
        ms["row_sumsq"] = timed(lambda: ops.row_sumsq(out, n_samples, out=energy))
        rate["row_sumsq"] = {"gb_per_s": 4.0 * n * B / (ms["row_sumsq"] * 1e-3) / 1e9}
        draws = [ops.augment_draw(SEED, b, 0, 0, 1000, bank.noise_len, SNR) for b in range(B)]
        mix = lambda: ops.noise_mix_rows(out, n_samples, energy, bank.noise_bank, bank.noise_len, bank.noise_sumsq,      # noqa: E731
                                         [d[1] for d in draws], [d[2] for d in draws], [d[3] for d in draws], out=out)
        plans["noise_mix_rows"] = ops.noise_mix_rows_plan(n_samples, n, bank.noise_len, bank.noise_bank.shape[1], [d[1] for d in draws],
                                                          [d[2] for d in draws], [d[3] for d in draws])
        ms["noise_mix_rows"] = timed(mix)
        rate["noise_mix_rows"] = {"gb_per_s": 12.0 * n * B / (ms["noise_mix_rows"] * 1e-3) / 1e9}      # row in, clip in, row out
        torch.cuda.synchronize()
        assert torch.isfinite(out).all()
        print(json.dumps({"launches": a.launches, "rows": B, "samples": n, "ms_per_call": ms, "rates": rate, "plans": plans}))
        return

    n = SR * SECONDS
    n_samples = [n] * B
    N_ROTATE = 4
    pcm_dev = [torch.from_numpy(np.stack([synth_pcm(k * B + b, n) for b in range(B)])).cuda() for k in range(N_ROTATE)]
    dlab = [torch.from_numpy(synth_labels(np.random.RandomState(100 + k))).cuda() for k in range(N_ROTATE)]
    bank = AugmentBank([synth_rir(a.taps, r) for r in range(8)], [synth_pcm(100 + m, SR * (3 + 2 * m)) * 0.2 for m in range(4)])
    nf = ops.frontend(pcm_dev[0], n_samples, SR, "mfcc", T, D)[1]
    lengths = torch.tensor([min(f, T) for f in nf], dtype=torch.int32).cuda()
    eng = Engine(L, H, D, C, B, T, U, seed=1234)
    torch.cuda.synchronize()
    torch.cuda.set_stream(eng.stream)          # a real (non-NULL) stream for the whole job (Engine.on_stream)
    side = torch.cuda.Stream()
    ahead = {}

    def prepare(on, i, after=None):
        """The pre-processing of step i on the side stream (bench.py's prefetch_features, with the stage in front)."""
        if after is not None:
            side.wait_event(after)
        with torch.cuda.stream(side):
            x = pcm_dev[i % N_ROTATE]
            if on:
                draws = [ops.augment_draw(SEED, (i << 32) | b, 1000, len(bank.rir_taps), 1000, bank.noise_len, SNR) for b in range(B)]
                x = ops.reverb_rows(x, n_samples, bank.rir_bank, bank.rir_taps, bank.rir_delay, [d[0] for d in draws])
                energy = ops.row_sumsq(x, n_samples)
                x = ops.noise_mix_rows(x, n_samples, energy, bank.noise_bank, bank.noise_len, bank.noise_sumsq, [d[1] for d in draws],
                                       [d[2] for d in draws], [d[3] for d in draws], out=x)
            f = ops.frontend(x, n_samples, SR, "mfcc", T, D)[0]
            ev = torch.cuda.Event()
            ev.record(side)
        ahead["f"], ahead["ev"] = f, ev
        return ev

    def step(on, i):
        if "f" not in ahead:
            prepare(on, i)
        x, ev = ahead.pop("f"), ahead.pop("ev")
        cur = torch.cuda.current_stream()
        cur.wait_event(ev)
        x.record_stream(cur)
        eng.zero_grads()
        eng.mini_batch(x, lengths, dlab[i % N_ROTATE], 0.8, 0.5, seed=i + 1, beside_forward=lambda after: prepare(on, i + 1, after))
        eng.apply(3e-4, 1.0)

    def window(on, w):
        ahead.clear()
        torch.cuda.synchronize()
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
    torch.cuda.synchronize()
    eng.check()
    loss = eng.loss.cpu().numpy()
    assert np.isfinite(loss).all() and (loss > 0).all()
    out = {"shape": "%dx%d, %d-dim mfcc, batch %d, %d s of %d Hz PCM, t_max %d, f32, dropout 0.8/0.5" % (L, H, D, B, SECONDS, SR, T),
           "taps": a.taps, "snr_decidb": SNR,
           "ms_per_step": {k: float(np.median(v)) for k, v in ms.items()},
           "ms_per_step_min_max": {k: [float(np.min(v)), float(np.max(v))] for k, v in ms.items()},
           "ratio": float(np.median(ms["on"]) / np.median(ms["off"])),
           "steps_per_window": a.steps, "windows": a.windows, "warmup_windows": a.warmup,
           "reverb_rows_plan": ops.reverb_rows_plan(n_samples, n, bank.rir_taps, bank.rir_delay, a.taps, [0] * B)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
